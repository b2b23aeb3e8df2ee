// Part of device.hip (single translation unit; see that file's header).  The weighted Gram pass: the plan and the launcher of
// kernels_gram.inc (DESIGN.md section 18).
// ----------------------------------------------------------------------------------------------
// Plan, a function of the dataset alone (its d and the tiles that hold its documents): the passes (diagonal ones first, each
// kind launched once with the passes as grid dimension y), the stretch of tiles a workgroup owns and hence the number of
// workgroups G.  G aims at three workgroups per compute unit and is cut where the slabs would exceed GRAM_SLAB_MAX.
struct GramState {
    bool built = false;
    uint32_t nbA = 0, nbB = 0, ndiag = 0, noff = 0, slots = 0, stretch = 0, G = 0, ntiles = 0;
    DevBuf<uint32_t> qof;
    DevBuf<unsigned char> qflags;
    DevBuf<GramPass> passes;  // [ndiag + noff]
    DevBuf<double> slab, out, lam_in, wt_in;
};

namespace {
constexpr uint32_t GRAM_TARGET_WORKGROUPS = 768;
constexpr size_t GRAM_SLAB_MAX = size_t(256) << 20;
constexpr size_t GRAM_LDS_DIAG = 128 * sizeof(double) + (size_t)64 * GRAM_PW * sizeof(float);
constexpr size_t GRAM_LDS_OFF = 128 * sizeof(double) + (size_t)2 * 64 * GRAM_PW * sizeof(float);
}  // namespace

template <typename ImplT>  // (DeviceDataset::Impl, which only members may name)
static bool gram_build(ImplT& m, std::string* err) {
    if (!m.gram) m.gram = std::make_shared<GramState>();
    GramState& gs = *m.gram;
    if (gs.built) return true;
    if (m.np % 64 != 0 || m.d == 0) {
        if (err) *err = "weighted_gram: the dataset has no whole tiles or no features";
        return false;
    }
    gs.nbA = (uint32_t)((m.d + 15) / 16), gs.nbB = (uint32_t)((m.d + 1 + 15) / 16);
    const uint32_t P = (gs.nbB + GRAM_PB - 1) / GRAM_PB;
    std::vector<GramPass> diag, off;
    for (uint32_t I = 0; I < P && I * GRAM_PB < gs.nbA; I++)
        for (uint32_t J = I; J < P; J++) (I == J ? diag : off).push_back(GramPass{I, J, 0u});
    gs.ndiag = (uint32_t)diag.size(), gs.noff = (uint32_t)off.size();
    diag.insert(diag.end(), off.begin(), off.end());
    for (size_t k = 0; k < diag.size(); k++) diag[k].index = (uint32_t)k;
    gs.slots = GRAM_WAVES * (gs.noff ? GRAM_OFF_SLOTS : GRAM_DIAG_SLOTS);
    gs.ntiles = (uint32_t)(m.nvtiles ? m.nvtiles : m.np / 64);
    const size_t per_wg = diag.size() * gs.slots * 256 * sizeof(double);
    const uint32_t gmax = (uint32_t)std::max<size_t>(1, std::min<size_t>(GRAM_TARGET_WORKGROUPS, GRAM_SLAB_MAX / per_wg));
    gs.stretch = std::max<uint32_t>(1, (gs.ntiles + gmax - 1) / gmax);
    gs.G = (gs.ntiles + gs.stretch - 1) / gs.stretch;
    // the query of every position (the view's own documents only)
    std::vector<uint32_t> qof(m.np, IDX_INVALID);
    for (size_t q = 0; q < m.nq; q++)
        for (uint32_t k = 0; k < m.qlen_h[q]; k++) qof[m.qstart_h[q] + k] = (uint32_t)q;
    if (!upload(gs.qof, qof, err) || !upload(gs.passes, diag, err)) return false;
    if (!gs.slab.ensure(std::max<size_t>(1, (size_t)gs.G * per_wg / sizeof(double)), err) || !gs.out.ensure(m.d * m.d + m.d, err)) return false;
    FR_HIP(hipFuncSetAttribute((const void*)weighted_gram_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GRAM_LDS_OFF));
    gs.built = true;
    return true;
}

bool DeviceDataset::weighted_gram(const double* lam_pos, const double* wt_pos, const unsigned char* query_flags, double* H, double* g,
                                  std::string* err, GramPlan* plan) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if ((lam_pos == nullptr) != (wt_pos == nullptr) || H == nullptr || g == nullptr) {
        if (err) *err = "weighted_gram: lambda and w come together, and both outputs are needed";
        return false;
    }
    if (lam_pos == nullptr && !m.lm.built) {
        if (err) *err = "weighted_gram: no gradients resident (run lambda_gradients first)";
        return false;
    }
    if (!gram_build(m, err)) return false;
    GramState& gs = *m.gram;
    if (gs.G == 0) {  // no tile holds a document: the sums are empty
        if (err) *err = "weighted_gram: the dataset holds no document";
        return false;
    }
    const double *lam = m.lm.lam.p, *wt = m.lm.wt.p;
    if (lam_pos != nullptr) {
        if (!gs.lam_in.ensure(m.np, err) || !gs.wt_in.ensure(m.np, err)) return false;
        FR_HIP(hipMemcpyAsync(gs.lam_in.p, lam_pos, m.np * sizeof(double), hipMemcpyHostToDevice, m.stream));
        FR_HIP(hipMemcpyAsync(gs.wt_in.p, wt_pos, m.np * sizeof(double), hipMemcpyHostToDevice, m.stream));
        lam = gs.lam_in.p, wt = gs.wt_in.p;
    }
    if (query_flags != nullptr) {
        if (!gs.qflags.ensure(std::max<size_t>(m.nq, 1), err)) return false;
        FR_HIP(hipMemcpyAsync(gs.qflags.p, query_flags, m.nq, hipMemcpyHostToDevice, m.stream));
    }
    GramArgs a;
    a.xb = (const float4*)m.xb.p;
    a.tiles = m.nvtiles ? m.vtiles.p : nullptr;
    a.ntiles = gs.ntiles, a.dq = (uint32_t)m.dq, a.d = (uint32_t)m.d, a.nbA = gs.nbA, a.nbB = gs.nbB, a.stretch = gs.stretch, a.slots = gs.slots;
    a.qof = gs.qof.p;
    a.qflags = query_flags != nullptr ? gs.qflags.p : nullptr;
    a.lam = lam, a.wt = wt;
    a.slab = gs.slab.p;
    {
        {
            ProfScope ps("weighted_gram_kernel", m.stream);
            weighted_gram_kernel<true><<<dim3(gs.G, gs.ndiag), 64 * GRAM_WAVES, GRAM_LDS_DIAG, m.stream>>>(a, gs.passes.p);
            if (gs.noff != 0)
                weighted_gram_kernel<false><<<dim3(gs.G, gs.noff), 64 * GRAM_WAVES, GRAM_LDS_OFF, m.stream>>>(a, gs.passes.p + gs.ndiag);
        }
        ProfScope ps("gram_fold_kernel", m.stream);
        gram_fold_kernel<<<dim3(gs.slots, gs.ndiag + gs.noff), 256, 0, m.stream>>>(gs.slab.p, gs.passes.p, gs.G, gs.slots, gs.nbA, gs.nbB, (uint32_t)m.d,
                                                                                   gs.out.p, gs.out.p + m.d * m.d);
    }
    FR_HIP(hipGetLastError());
    FR_HIP(hipMemcpyAsync(H, gs.out.p, m.d * m.d * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(g, gs.out.p + m.d * m.d, m.d * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    if (plan != nullptr) {
        plan->blocks_a = gs.nbA, plan->blocks_b = gs.nbB, plan->passes = gs.ndiag + gs.noff, plan->stretch = gs.stretch;
        plan->workgroups = gs.G, plan->tiles = gs.ntiles;
        plan->slab_bytes = (uint64_t)gs.slab.bytes();
        plan->tile_bytes = (uint64_t)gs.ntiles * m.dq * 256 * sizeof(float);
    }
    return true;
}

