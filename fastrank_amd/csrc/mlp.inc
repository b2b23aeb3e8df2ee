// Part of device.hip (single translation unit; see that file's header).  The one-hidden-layer net's scoring and
// back-propagation: the plan, the packing of the parameters and the launchers of kernels_mlp.inc (DESIGN.md section 19).
// ----------------------------------------------------------------------------------------------
// Plan.  nfp = ceil(d / 144) feature panels, nhp = ceil(h / 64) hidden panels.  The stretch of tiles a workgroup owns aims at
// three workgroups per compute unit: it is a function of the dataset alone, except that back-propagation lengthens it where
// the records of nhp * nfp passes would exceed MLP_SLAB_MAX (never at d <= 144 and h <= 64 * 5).  W1 is packed on the host
// into the B fragments the kernels read: wf[hp][fp][ks][wave][lane] = W1[64 hp + 16 wave + lane % 16][144 fp + 4 ks + lane / 16],
// zero outside the model.
struct MlpState {
    bool built = false;
    uint32_t ntiles = 0, nfp = 0;
    DevBuf<uint32_t> qof;
    DevBuf<unsigned char> qflags;
    DevBuf<double> wf, bias, slab, out, lam_in;  // bias: b1 | w2, each zero-padded to nhp * 64
};

namespace {
constexpr uint32_t MLP_TARGET_WORKGROUPS = 768;
constexpr size_t MLP_SLAB_MAX = size_t(256) << 20;
constexpr size_t MLP_LDS_RES = 64 * sizeof(double) + (size_t)64 * MLP_ROW * sizeof(float);
constexpr size_t MLP_LDS_GEN = 64 * sizeof(double) + (size_t)2 * 64 * MLP_ROW * sizeof(float);
constexpr size_t MLP_MAX_SIDE = 1024;  // (tested up to here; nothing below it is refused)
}  // namespace

template <typename ImplT>  // (DeviceDataset::Impl, which only members may name)
static bool mlp_build(ImplT& m, std::string* err) {
    if (!m.mlp) m.mlp = std::make_shared<MlpState>();
    MlpState& ms = *m.mlp;
    if (ms.built) return true;
    if (m.np % 64 != 0 || m.d == 0) {
        if (err) *err = "NeuralNet: the dataset has no whole tiles or no features";
        return false;
    }
    ms.nfp = (uint32_t)((m.d + MLP_FP - 1) / MLP_FP);
    ms.ntiles = (uint32_t)(m.nvtiles ? m.nvtiles : m.np / 64);
    std::vector<uint32_t> qof(m.np, IDX_INVALID);  // the query of every position (the view's own documents only)
    for (size_t q = 0; q < m.nq; q++)
        for (uint32_t k = 0; k < m.qlen_h[q]; k++) qof[m.qstart_h[q] + k] = (uint32_t)q;
    if (!upload(ms.qof, qof, err)) return false;
    FR_HIP(hipFuncSetAttribute((const void*)mlp_backprop_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MLP_LDS_GEN));
    ms.built = true;
    return true;
}

// wf[hp][fp][ks][wave][lane] (the header) from the first `cols` columns of W1's h rows of dm numbers
static std::vector<double> mlp_pack_w1(uint32_t nfp, size_t h, size_t dm, size_t cols, const double* W1) {
    std::vector<double> wf((h + MLP_HP - 1) / MLP_HP * nfp * MLP_FRAG, 0.0);
    for (size_t j = 0; j < h; j++) {
        const size_t hp = j / MLP_HP, wave = (j % MLP_HP) / 16, c = j % 16;
        for (size_t i = 0; i < cols; i++) {
            const size_t fp = i / MLP_FP, ks = (i % MLP_FP) / 4, k = i % 4;
            wf[(hp * nfp + fp) * MLP_FRAG + (ks * MLP_WAVES + wave) * 64 + 16 * k + c] = W1[j * dm + i];
        }
    }
    return wf;
}

// the parameters as the kernels read them; fills the plan's shape.  W1: h rows of dm numbers (columns >= d are not read).
template <typename ImplT>
static bool mlp_upload(ImplT& m, size_t h, size_t dm, const double* W1, const double* b1, const double* w2, uint32_t* nhp_out, std::string* err) {
    MlpState& ms = *m.mlp;
    if (h == 0 || h > MLP_MAX_SIDE || W1 == nullptr || b1 == nullptr || w2 == nullptr) {
        if (err) *err = "NeuralNet: the kernels take 1 to " + std::to_string(MLP_MAX_SIDE) + " hidden units";
        return false;
    }
    const uint32_t nhp = (uint32_t)((h + MLP_HP - 1) / MLP_HP), nfp = ms.nfp;
    std::vector<double> wf = mlp_pack_w1(nfp, h, dm, std::min(dm, m.d), W1), bias((size_t)2 * nhp * MLP_HP, 0.0);
    for (size_t j = 0; j < h; j++) bias[j] = b1[j], bias[(size_t)nhp * MLP_HP + j] = w2[j];
    if (!ms.wf.ensure(wf.size(), err) || !ms.bias.ensure(bias.size(), err)) return false;
    FR_HIP(hipMemcpyAsync(ms.wf.p, wf.data(), wf.size() * sizeof(double), hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemcpyAsync(ms.bias.p, bias.data(), bias.size() * sizeof(double), hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));  // (wf and bias are locals)
    *nhp_out = nhp;
    return true;
}

template <typename ImplT>
static MlpArgs mlp_args(ImplT& m, uint32_t nhp, uint32_t stretch, double b2) {
    MlpState& ms = *m.mlp;
    MlpArgs a;
    a.xb = (const float4*)m.xb.p;
    a.tiles = m.nvtiles ? m.vtiles.p : nullptr;
    a.ntiles = ms.ntiles, a.dq = (uint32_t)m.dq, a.nfp = ms.nfp, a.nhp = nhp, a.stretch = stretch;
    a.qof = ms.qof.p, a.qflags = nullptr;
    a.wf = ms.wf.p, a.b1 = ms.bias.p, a.w2 = ms.bias.p + (size_t)nhp * MLP_HP, a.b2 = b2;
    a.lam = nullptr, a.scores = nullptr, a.slab = nullptr;
    return a;
}

bool DeviceDataset::score_mlp(size_t h, size_t dm, const double* W1, const double* b1, const double* w2, double b2, std::string* err, MlpPlan* plan) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (!m.scores.ensure(std::max<size_t>(m.np, 1), err)) return false;
    m.scores_slots = 1;
    if (m.np == 0) return true;
    uint32_t nhp = 0;
    if (!mlp_build(m, err) || !mlp_upload(m, h, dm, W1, b1, w2, &nhp, err)) return false;
    MlpState& ms = *m.mlp;
    const uint32_t stretch = std::max<uint32_t>(1, (ms.ntiles + MLP_TARGET_WORKGROUPS - 1) / MLP_TARGET_WORKGROUPS);
    const uint32_t G = (ms.ntiles + stretch - 1) / stretch;
    const bool res = ms.nfp == 1 && nhp == 1;
    if (G != 0) {
        MlpArgs a = mlp_args(m, nhp, stretch, b2);
        a.scores = m.scores.p;
        ProfScope ps("mlp_score_kernel", m.stream);
        if (res)
            mlp_score_kernel<true><<<G, 64 * MLP_WAVES, 0, m.stream>>>(a);
        else
            mlp_score_kernel<false><<<G, 64 * MLP_WAVES, 0, m.stream>>>(a);
    }
    FR_HIP(hipGetLastError());
    if (plan != nullptr) {
        plan->feature_panels = ms.nfp, plan->hidden_panels = nhp, plan->stretch = stretch, plan->workgroups = G, plan->tiles = ms.ntiles;
        plan->resident = res, plan->slab_bytes = 0;
        plan->tile_bytes = (uint64_t)ms.ntiles * m.dq * 256 * sizeof(float);
    }
    return true;
}

bool DeviceDataset::mlp_backprop(size_t h, size_t dm, const double* W1, const double* b1, const double* w2, const double* lam_pos,
                                 const unsigned char* query_flags, double* g_w1, double* g_b1, double* g_w2, double* g_b2, std::string* err,
                                 MlpPlan* plan) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (g_w1 == nullptr || g_b1 == nullptr || g_w2 == nullptr || g_b2 == nullptr) {
        if (err) *err = "mlp_backprop: all four outputs are needed";
        return false;
    }
    if (lam_pos == nullptr && !m.lm.built) {
        if (err) *err = "mlp_backprop: no gradients resident (run lambda_gradients first)";
        return false;
    }
    uint32_t nhp = 0;
    if (!mlp_build(m, err) || !mlp_upload(m, h, dm, W1, b1, w2, &nhp, err)) return false;
    MlpState& ms = *m.mlp;
    if (ms.ntiles == 0) {
        if (err) *err = "mlp_backprop: the dataset holds no document";
        return false;
    }
    const uint32_t passes = nhp * ms.nfp;
    const size_t per_wg = (size_t)passes * MLP_REC * sizeof(double);
    const uint32_t gmax = (uint32_t)std::max<size_t>(1, std::min<size_t>(MLP_TARGET_WORKGROUPS, MLP_SLAB_MAX / per_wg));
    const uint32_t stretch = std::max<uint32_t>(1, (ms.ntiles + gmax - 1) / gmax), G = (ms.ntiles + stretch - 1) / stretch;
    const size_t nout = h * m.d + 2 * h + 1;
    if (!ms.slab.ensure((size_t)G * passes * MLP_REC, err) || !ms.out.ensure(nout, err)) return false;
    MlpArgs a = mlp_args(m, nhp, stretch, 0.0);
    a.lam = m.lm.lam.p;
    if (lam_pos != nullptr) {
        if (!ms.lam_in.ensure(m.np, err)) return false;
        FR_HIP(hipMemcpyAsync(ms.lam_in.p, lam_pos, m.np * sizeof(double), hipMemcpyHostToDevice, m.stream));
        a.lam = ms.lam_in.p;
    }
    if (query_flags != nullptr) {
        if (!ms.qflags.ensure(std::max<size_t>(m.nq, 1), err)) return false;
        FR_HIP(hipMemcpyAsync(ms.qflags.p, query_flags, m.nq, hipMemcpyHostToDevice, m.stream));
        a.qflags = ms.qflags.p;
    }
    a.slab = ms.slab.p;
    const bool res = ms.nfp == 1;
    {
        {
            ProfScope ps("mlp_backprop_kernel", m.stream);
            if (res)
                mlp_backprop_kernel<true><<<dim3(G, passes), 64 * MLP_WAVES, MLP_LDS_RES, m.stream>>>(a);
            else
                mlp_backprop_kernel<false><<<dim3(G, passes), 64 * MLP_WAVES, MLP_LDS_GEN, m.stream>>>(a);
        }
        ProfScope ps("mlp_fold_kernel", m.stream);
        mlp_fold_kernel<<<(unsigned)((nout + 255) / 256), 256, 0, m.stream>>>(ms.slab.p, G, ms.nfp, (uint32_t)h, (uint32_t)m.d, ms.out.p);
    }
    FR_HIP(hipGetLastError());
    const size_t nw = h * m.d;
    FR_HIP(hipMemcpyAsync(g_w1, ms.out.p, nw * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(g_b1, ms.out.p + nw, h * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(g_w2, ms.out.p + nw + h, h * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(g_b2, ms.out.p + nw + 2 * h, sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    if (plan != nullptr) {
        plan->feature_panels = ms.nfp, plan->hidden_panels = nhp, plan->stretch = stretch, plan->workgroups = G, plan->tiles = ms.ntiles;
        plan->resident = res, plan->slab_bytes = (uint64_t)G * per_wg;
        plan->tile_bytes = (uint64_t)ms.ntiles * m.dq * 256 * sizeof(float);
    }
    return true;
}

