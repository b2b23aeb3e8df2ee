// Part of device.hip (single translation unit; see that file's header).  LambdaMART's gradient pass: the launchers of kernels_lambda.inc and kernels_xendcg.inc.
// ----------------------------------------------------------------------------------------------
// LambdaMART gradient pass (kernels_lambda.inc, kernels_xendcg.inc)
// ----------------------------------------------------------------------------------------------
// per query the positions of its documents in stored order (instance ids ascending), and the launch order (longest first)
bool DeviceDataset::Impl::lm_build(std::string* err) {
    if (lm.built) return true;
    std::vector<uint32_t> off(nq + 1, 0), pos, order(nq);
    pos.reserve(n);
    uint32_t maxl = 0;
    for (size_t q = 0; q < nq; q++) {
        const size_t b = pos.size();
        for (uint32_t k = 0; k < qlen_h[q]; k++) pos.push_back(qstart_h[q] + k);
        std::sort(pos.begin() + b, pos.end(), [&](uint32_t x, uint32_t y) { return perm_host[x] < perm_host[y]; });
        off[q + 1] = (uint32_t)pos.size();
        maxl = std::max(maxl, qlen_h[q]);
        order[q] = (uint32_t)q;
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return qlen_h[a] > qlen_h[b]; });
    // queries beyond the LDS budget (4096 documents, 144 KiB) are staged in a per-block global slab; they come first in
    // the longest-first order
    uint32_t n_long = 0;
    while (n_long < nq && (size_t)qlen_h[order[n_long]] * LM_STAGE_BYTES > LM_LDS_MAX) n_long++;
    if (!upload(lm.off, off, err) || !upload(lm.pos, pos, err) || !upload(lm.qorder, order, err)) return false;
    if (!lm.lam.ensure(np, err) || !lm.wt.ensure(np, err) || !lm.target.ensure(np, err)) return false;
    FR_HIP(hipMemsetAsync(lm.lam.p, 0, np * sizeof(double), stream));
    FR_HIP(hipMemsetAsync(lm.wt.p, 0, np * sizeof(double), stream));
    FR_HIP(hipMemsetAsync(lm.target.p, 0, np * sizeof(float), stream));
    lm.n_lds = (uint32_t)nq - n_long;
    lm.max_len = maxl;
    lm.order_h = order;
    if (n_long && !lm.slab.ensure((size_t)LM_SLAB_BLOCKS * maxl * LM_STAGE_BYTES, err)) return false;
    lm.built = true;
    return true;
}

bool DeviceDataset::lambda_gradients(const double* norms, int64_t depth, double sigma, const LambdaPass& pass, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (m.scores_slots < 1 || m.scores.p == nullptr) {
        if (err) *err = "lambda_gradients: no scores resident";
        return false;
    }
    if (pass.objective < LM_OBJ_NDCG || pass.objective > LM_OBJ_XENDCG) {
        if (err) *err = "lambda_gradients: unknown objective " + std::to_string(pass.objective);
        return false;
    }
    if (pass.objective == LM_OBJ_XENDCG && (pass.truncation_level != 0 || pass.lambda_norm)) {
        if (err) *err = "lambda_gradients: the listwise objective has no pairs to truncate or normalise";
        return false;
    }
    if (!m.lm_build(err)) return false;
    if (!m.norms.ensure(m.nq, err) || !m.upload_norms(norms, err)) return false;
    auto& lm = m.lm;
    uint32_t n_long = (uint32_t)m.nq - lm.n_lds, n_lds = lm.n_lds;
    const uint32_t* qorder = lm.qorder.p;
    size_t longest = n_long < m.nq ? std::min<size_t>(lm.max_len, LM_LDS_MAX / LM_STAGE_BYTES) : 0;
    if (pass.query_flags != nullptr) {  // a tree's query sample: qorder filtered, its order kept (slab queries still open the pass)
        if (!(pass.flags_unchanged && lm.qsel_valid)) {
            lm.qsel_valid = false;
            lm.qsel_h.clear();
            lm.sel_long = 0;
            for (size_t i = 0; i < m.nq; i++) {
                const uint32_t q = lm.order_h[i];
                if (!pass.query_flags[q]) continue;
                if (i < n_long) lm.sel_long++;
                lm.qsel_h.push_back(q);
            }
            if (lm.qsel_h.empty()) return true;
            if (!lm.qsel.ensure(m.nq, err)) return false;
            FR_HIP(hipMemcpyAsync(lm.qsel.p, lm.qsel_h.data(), lm.qsel_h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, m.stream));
            lm.qsel_valid = true;
        }
        const uint32_t sel_long = lm.sel_long;
        n_long = sel_long, n_lds = (uint32_t)lm.qsel_h.size() - sel_long;
        qorder = lm.qsel.p;
        longest = n_lds ? m.qlen_h[lm.qsel_h[n_long]] : 0;  // (the longest sampled query that is staged in LDS)
    }
    if (pass.objective == LM_OBJ_XENDCG) {  // DESIGN.md section 11, "Listwise objective": one wave per query, long queries included
        const uint32_t n_q = n_long + n_lds;
        if (n_q == 0) return true;
        ProfScope ps("lambda_grad_xe_kernel", m.stream);
        lambda_grad_xe_kernel<<<(n_q + XE_WAVES - 1) / XE_WAVES, 64 * XE_WAVES, 0, m.stream>>>(
            m.scores.p, lm.off.p, lm.pos.p, qorder, n_q, m.gexp.p, m.perm.p, m.norms.p, pass.xe_key, lm.lam.p, lm.wt.p, lm.target.p);
        FR_HIP(hipGetLastError());
        return true;
    }
    if (pass.truncation_level != 0 || pass.lambda_norm) {  // DESIGN.md section 11, "Truncation and normalisation": a kernel of its own
        const uint32_t trunc = pass.truncation_level != 0 ? pass.truncation_level : 0xFFFFFFFFu;  // (no level: every rank is inside)
        if (pass.lambda_norm && !lm.asum.ensure(m.np, err)) return false;
        ProfScope ps("lambda_grad_trunc_kernel", m.stream);
        auto* const kernel = pass.objective == LM_OBJ_MAP ? lambda_grad_trunc_kernel<LM_OBJ_MAP>
                             : pass.objective == LM_OBJ_MRR ? lambda_grad_trunc_kernel<LM_OBJ_MRR> : lambda_grad_trunc_kernel<LM_OBJ_NDCG>;
        for (uint32_t q0 = 0; q0 < n_long; q0 += LM_SLAB_BLOCKS) {
            const uint32_t cnt = std::min<uint32_t>(LM_SLAB_BLOCKS, n_long - q0);
            kernel<<<cnt, 256, 0, m.stream>>>(m.scores.p, lm.off.p, lm.pos.p, qorder, q0, m.gain.p, m.gexp.p, m.disc.p, m.perm.p, m.norms.p,
                                              depth, sigma, trunc, pass.lambda_norm ? 1 : 0, lm.lam.p, lm.wt.p, lm.target.p, lm.asum.p, lm.slab.p,
                                              lm.max_len);
        }
        if (n_lds != 0) {
            const size_t bytes = std::max<size_t>(longest * LM_STAGE_BYTES, 64);
            FR_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
            kernel<<<n_lds, 256, bytes, m.stream>>>(m.scores.p, lm.off.p, lm.pos.p, qorder, n_long, m.gain.p, m.gexp.p, m.disc.p, m.perm.p,
                                                    m.norms.p, depth, sigma, trunc, pass.lambda_norm ? 1 : 0, lm.lam.p, lm.wt.p, lm.target.p,
                                                    lm.asum.p, nullptr, 0u);
        }
        FR_HIP(hipGetLastError());
        return true;
    }
    ProfScope ps("lambda_grad_kernel", m.stream);
    auto* const kernel = pass.objective == LM_OBJ_MAP ? lambda_grad_kernel<LM_OBJ_MAP>
                         : pass.objective == LM_OBJ_MRR ? lambda_grad_kernel<LM_OBJ_MRR> : lambda_grad_kernel<LM_OBJ_NDCG>;
    for (uint32_t q0 = 0; q0 < n_long; q0 += LM_SLAB_BLOCKS) {  // (longest first: these open the pass)
        const uint32_t cnt = std::min<uint32_t>(LM_SLAB_BLOCKS, n_long - q0);
        kernel<<<cnt, 256, 0, m.stream>>>(m.scores.p, lm.off.p, lm.pos.p, qorder, q0, m.gain.p, m.gexp.p, m.disc.p, m.perm.p, m.norms.p, depth,
                                          sigma, lm.lam.p, lm.wt.p, lm.target.p, lm.slab.p, lm.max_len);
    }
    if (n_lds != 0) {
        const size_t bytes = std::max<size_t>(longest * LM_STAGE_BYTES, 64);
        FR_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        kernel<<<n_lds, 256, bytes, m.stream>>>(m.scores.p, lm.off.p, lm.pos.p, qorder, n_long, m.gain.p, m.gexp.p, m.disc.p, m.perm.p,
                                                m.norms.p, depth, sigma, lm.lam.p, lm.wt.p, lm.target.p, nullptr, 0u);
    }
    FR_HIP(hipGetLastError());
    return true;
}

bool DeviceDataset::lambda_download_positions(std::vector<double>* lambda, std::vector<double>* weight, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (!m.lm.built) {
        if (err) *err = "lambda_download: no gradients computed";
        return false;
    }
    lambda->resize(m.np);
    weight->resize(m.np);
    FR_HIP(hipMemcpyAsync(lambda->data(), m.lm.lam.p, m.np * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(weight->data(), m.lm.wt.p, m.np * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    return true;
}

bool DeviceDataset::lambda_download(double* lambda_by_instance, double* weight_by_instance, size_t out_len, std::string* err,
                                    const unsigned char* query_flags) {
    std::vector<double> lam, wt;
    if (!lambda_download_positions(&lam, &wt, err)) return false;
    Impl& m = *impl_;
    std::vector<char> in_query(m.np, 0);
    for (size_t q = 0; q < m.nq; q++) {
        if (query_flags != nullptr && !query_flags[q]) continue;
        for (uint32_t k = 0; k < m.qlen_h[q]; k++) in_query[m.qstart_h[q] + k] = 1;
    }
    for (size_t p = 0; p < m.np; p++) {
        const uint32_t id = m.perm_host[p];
        if (!in_query[p] || id == IDX_INVALID || id >= out_len) continue;
        lambda_by_instance[id] = lam[p];
        weight_by_instance[id] = wt[p];
    }
    return true;
}

