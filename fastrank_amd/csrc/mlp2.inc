// Part of device.hip (single translation unit; see that file's header).  The two-hidden-layer net's scoring and
// back-propagation: the packing of the parameters and the launchers of kernels_mlp2.inc (DESIGN.md section 19, "Two hidden
// layers").  Plan, tables and the packing of W1 are mlp.inc's.
// ----------------------------------------------------------------------------------------------
// W2 is packed twice, each time into the B fragments of one product, zero outside the model:
//   w2f[hp][kk][wave][lane] = W2[16 wave + lane % 16][64 hp + 4 kk + lane / 16]     (z2 = a1 W2^T: contracts over first-layer units)
//   w2b[hp][kk][wave][lane] = W2[4 kk + lane / 16][64 hp + 16 wave + lane % 16]     (e = d2 W2: contracts over second-layer units)
// W1's fragments stay in registers for scoring with one feature panel and one hidden panel; back-propagation reads them per step.
struct Mlp2State {
    bool built = false;
    DevBuf<double> wf, par, w2f, w2b, slab, out;  // par: b1 zero-padded to nhp * 64 | c | w3, each zero-padded to 64
};

namespace {
constexpr size_t MLP2_MAX_HIDDEN2 = MLP_HP;
constexpr size_t MLP2_LDS_SCORE = ((size_t)64 * MLP2_ROW + MLP_WAVES * 64) * sizeof(double) + (size_t)64 * MLP_ROW * sizeof(float);
constexpr size_t MLP2_LDS_ONE = ((size_t)64 * MLP2_ROW + 64) * sizeof(double) + (size_t)64 * MLP_ROW * sizeof(float);
constexpr size_t MLP2_LDS_GEN = MLP2_LDS_ONE + (size_t)64 * MLP_ROW * sizeof(float);
}  // namespace

template <typename ImplT>
static bool mlp2_upload(ImplT& m, const DeviceDataset::Mlp2Net& n, uint32_t* nhp_out, std::string* err) {
    if (!m.mlp2) m.mlp2 = std::make_shared<Mlp2State>();
    Mlp2State& s2 = *m.mlp2;
    if (n.h == 0 || n.h > MLP_MAX_SIDE || n.h2 == 0 || n.h2 > MLP2_MAX_HIDDEN2 || !n.W1 || !n.b1 || !n.W2 || !n.c || !n.w3) {
        if (err)
            *err = "NeuralNet: the kernels take 1 to " + std::to_string(MLP_MAX_SIDE) + " units in the first hidden layer and 1 to " +
                   std::to_string(MLP2_MAX_HIDDEN2) + " in the second";
        return false;
    }
    if (!s2.built) {
        FR_HIP(hipFuncSetAttribute((const void*)mlp2_score_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MLP2_LDS_SCORE));
        FR_HIP(hipFuncSetAttribute((const void*)mlp2_score_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MLP2_LDS_SCORE));
        FR_HIP(hipFuncSetAttribute((const void*)mlp2_backprop_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MLP2_LDS_GEN));
        s2.built = true;
    }
    const size_t h = n.h, h2 = n.h2, nhp = (h + MLP_HP - 1) / MLP_HP;
    const std::vector<double> wf = mlp_pack_w1(m.mlp->nfp, h, n.dm, std::min(n.dm, m.d), n.W1);
    std::vector<double> par((nhp + 2) * MLP_HP, 0.0), w2f(nhp * MLP2_FRAG, 0.0), w2b(nhp * MLP2_FRAG, 0.0);
    std::copy(n.b1, n.b1 + h, par.begin());
    std::copy(n.c, n.c + h2, par.begin() + nhp * MLP_HP);
    std::copy(n.w3, n.w3 + h2, par.begin() + (nhp + 1) * MLP_HP);
    for (size_t k = 0; k < h2; k++)
        for (size_t j = 0; j < h; j++) {
            const size_t hp = j / MLP_HP, u = j % MLP_HP;
            w2f[hp * MLP2_FRAG + ((u / 4) * MLP_WAVES + k / 16) * 64 + 16 * (u % 4) + k % 16] = n.W2[k * h + j];
            w2b[hp * MLP2_FRAG + ((k / 4) * MLP_WAVES + u / 16) * 64 + 16 * (k % 4) + u % 16] = n.W2[k * h + j];
        }
    const std::pair<DevBuf<double>*, const std::vector<double>*> ups[] = {{&s2.wf, &wf}, {&s2.par, &par}, {&s2.w2f, &w2f}, {&s2.w2b, &w2b}};
    for (const auto& up : ups) {
        if (!up.first->ensure(up.second->size(), err)) return false;
        FR_HIP(hipMemcpyAsync(up.first->p, up.second->data(), up.second->size() * sizeof(double), hipMemcpyHostToDevice, m.stream));
    }
    FR_HIP(hipStreamSynchronize(m.stream));  // (the vectors are locals)
    *nhp_out = (uint32_t)nhp;
    return true;
}

template <typename ImplT>
static Mlp2Args mlp2_args(ImplT& m, const DeviceDataset::Mlp2Net& n, uint32_t nhp, uint32_t stretch) {
    MlpState& ms = *m.mlp;
    Mlp2State& s2 = *m.mlp2;
    Mlp2Args a;
    a.m.xb = (const float4*)m.xb.p;
    a.m.tiles = m.nvtiles ? m.vtiles.p : nullptr;
    a.m.ntiles = ms.ntiles, a.m.dq = (uint32_t)m.dq, a.m.nfp = ms.nfp, a.m.nhp = nhp, a.m.stretch = stretch;
    a.m.qof = ms.qof.p, a.m.qflags = nullptr;
    a.m.wf = s2.wf.p, a.m.b1 = s2.par.p, a.m.w2 = s2.par.p + (size_t)(nhp + 1) * MLP_HP, a.m.b2 = n.b_out;
    a.m.lam = nullptr, a.m.scores = nullptr, a.m.slab = nullptr;
    a.w2f = s2.w2f.p, a.w2b = s2.w2b.p, a.c = s2.par.p + (size_t)nhp * MLP_HP;
    a.h = (uint32_t)n.h, a.h2 = (uint32_t)n.h2;
    return a;
}

static void mlp2_plan(const MlpState& ms, const DeviceDataset::Mlp2Net& n, uint32_t nhp, uint32_t stretch, uint32_t G, bool resident,
                      uint64_t slab_bytes, size_t dq, DeviceDataset::MlpPlan* plan) {
    if (plan == nullptr) return;
    plan->feature_panels = ms.nfp, plan->hidden_panels = nhp, plan->stretch = stretch, plan->workgroups = G, plan->tiles = ms.ntiles;
    plan->hidden2 = (uint32_t)n.h2;
    plan->resident = resident, plan->slab_bytes = slab_bytes;
    plan->tile_bytes = (uint64_t)ms.ntiles * dq * 256 * sizeof(float);
}

bool DeviceDataset::score_mlp2(const Mlp2Net& net, std::string* err, MlpPlan* plan) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (!m.scores.ensure(std::max<size_t>(m.np, 1), err)) return false;
    m.scores_slots = 1;
    if (m.np == 0) return true;
    uint32_t nhp = 0;
    if (!mlp_build(m, err) || !mlp2_upload(m, net, &nhp, err)) return false;
    MlpState& ms = *m.mlp;
    const uint32_t stretch = std::max<uint32_t>(1, (ms.ntiles + MLP_TARGET_WORKGROUPS - 1) / MLP_TARGET_WORKGROUPS);
    const uint32_t G = (ms.ntiles + stretch - 1) / stretch;
    if (G != 0) {
        Mlp2Args a = mlp2_args(m, net, nhp, stretch);
        a.m.scores = m.scores.p;
        ProfScope ps("mlp2_score_kernel", m.stream);
        if (ms.nfp == 1 && nhp == 1)
            mlp2_score_kernel<true><<<G, 64 * MLP_WAVES, MLP2_LDS_SCORE, m.stream>>>(a);
        else
            mlp2_score_kernel<false><<<G, 64 * MLP_WAVES, MLP2_LDS_SCORE, m.stream>>>(a);
    }
    FR_HIP(hipGetLastError());
    mlp2_plan(ms, net, nhp, stretch, G, ms.nfp == 1 && nhp == 1, 0, m.dq, plan);
    return true;
}

bool DeviceDataset::mlp2_backprop(const Mlp2Net& net, const double* lam_pos, const unsigned char* query_flags, double* grad, std::string* err,
                                  MlpPlan* plan) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (grad == nullptr) {
        if (err) *err = "mlp2_backprop: the output is needed";
        return false;
    }
    if (lam_pos == nullptr && !m.lm.built) {
        if (err) *err = "mlp2_backprop: no gradients resident (run lambda_gradients first)";
        return false;
    }
    uint32_t nhp = 0;
    if (!mlp_build(m, err) || !mlp2_upload(m, net, &nhp, err)) return false;
    MlpState& ms = *m.mlp;
    Mlp2State& s2 = *m.mlp2;
    if (ms.ntiles == 0) {
        if (err) *err = "mlp2_backprop: the dataset holds no document";
        return false;
    }
    const uint32_t passes = nhp * ms.nfp;
    const size_t per_wg = (size_t)passes * MLP2_REC * sizeof(double);
    const uint32_t gmax = (uint32_t)std::max<size_t>(1, std::min<size_t>(MLP_TARGET_WORKGROUPS, MLP_SLAB_MAX / per_wg));
    const uint32_t stretch = std::max<uint32_t>(1, (ms.ntiles + gmax - 1) / gmax), G = (ms.ntiles + stretch - 1) / stretch;
    const size_t nout = net.h * m.d + net.h + net.h2 * net.h + 2 * net.h2 + 1;
    if (!s2.slab.ensure((size_t)G * passes * MLP2_REC, err) || !s2.out.ensure(nout, err)) return false;
    Mlp2Args a = mlp2_args(m, net, nhp, stretch);
    a.m.lam = m.lm.lam.p;
    if (lam_pos != nullptr) {
        if (!ms.lam_in.ensure(m.np, err)) return false;
        FR_HIP(hipMemcpyAsync(ms.lam_in.p, lam_pos, m.np * sizeof(double), hipMemcpyHostToDevice, m.stream));
        a.m.lam = ms.lam_in.p;
    }
    if (query_flags != nullptr) {
        if (!ms.qflags.ensure(std::max<size_t>(m.nq, 1), err)) return false;
        FR_HIP(hipMemcpyAsync(ms.qflags.p, query_flags, m.nq, hipMemcpyHostToDevice, m.stream));
        a.m.qflags = ms.qflags.p;
    }
    a.m.slab = s2.slab.p;
    {
        {
            ProfScope ps("mlp2_backprop_kernel", m.stream);
            mlp2_backprop_kernel<<<dim3(G, passes), 64 * MLP_WAVES, ms.nfp == 1 ? MLP2_LDS_ONE : MLP2_LDS_GEN, m.stream>>>(a);
        }
        ProfScope ps("mlp2_fold_kernel", m.stream);
        mlp2_fold_kernel<<<(unsigned)((nout + 255) / 256), 256, 0, m.stream>>>(s2.slab.p, G, ms.nfp, (uint32_t)net.h, (uint32_t)net.h2, (uint32_t)m.d,
                                                                                s2.out.p);
    }
    FR_HIP(hipGetLastError());
    FR_HIP(hipMemcpyAsync(grad, s2.out.p, nout * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    mlp2_plan(ms, net, nhp, stretch, G, false, (uint64_t)G * per_wg, m.dq, plan);
    return true;
}
