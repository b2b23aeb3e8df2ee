// Part of device.hip (single translation unit; see that file's header).  LambdaMART's histogram grower, level-wise and leaf-wise: the launchers of kernels_hist.inc.
// ----------------------------------------------------------------------------------------------
// LambdaMART histogram grower (kernels_hist.inc)
// ----------------------------------------------------------------------------------------------
static bool hist_fail(std::string* err, const std::string& what) {
    if (err) *err = "LambdaMART histogram grower: " + what;
    return false;
}

bool DeviceDataset::hist_bins(const uint32_t* positions, size_t n, const std::vector<uint32_t>& feats, uint32_t k, bool* built,
                              std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    if (built) *built = false;
    if (k < 2 || k > HIST_MAX_BINS) return hist_fail(err, "split_candidates must be between 2 and 256");
    if (n == 0 || feats.empty()) return hist_fail(err, "no instances or no features");
    if (n >= (1ull << 31)) return hist_fail(err, "more instances than the index list can hold");
    for (uint32_t f : feats)
        if (f >= m.d) return hist_fail(err, "feature id outside the dataset");
    if (h.k == k && h.n == n && h.feats == feats && std::equal(h.pos_host.begin(), h.pos_host.end(), positions)) {
        h.nt = h.n, h.Ft = h.F, h.q_sampled = h.f_sampled = h.g_on = h.qz_on = false;  // (no sample until hist_sample says so)
        return true;
    }
    h.k = 0;  // (nothing valid until the end of this function)
    const size_t F = feats.size();
    for (size_t i = 0; i < n; i++)
        if (positions[i] >= m.np) return hist_fail(err, "instance position outside the dataset");
    {
        const size_t need = F * n + 3 * n * sizeof(float) + ((size_t)64 << 20), have = device_free_bytes() + h.xbin.bytes();
        if (have != h.xbin.bytes() && have < need)
            return hist_fail(err, "the bin matrix needs " + std::to_string(need >> 20) + " MB of device memory, " +
                                      std::to_string(have >> 20) + " MB are free");
    }
    h.pos_host.assign(positions, positions + n);
    if (!h.pos.ensure(n, err) || !h.xbin.ensure(F * n, err) || !h.edges.ensure(F * HIST_MAX_BINS, err) || !h.nedges.ensure(F, err)) return false;
    DevBuf<float> col, sorted, firsts;
    DevBuf<uint32_t> count;
    DevBuf<int> nan_flag;
    if (!col.ensure(n, err) || !sorted.ensure(n, err) || !firsts.ensure(F * (HIST_MAX_BINS + 1), err) || !count.ensure(F, err) || !nan_flag.ensure(1, err))
        return false;
    FR_HIP(hipMemcpyAsync(h.pos.p, h.pos_host.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemsetAsync(count.p, 0, F * sizeof(uint32_t), m.stream));
    FR_HIP(hipMemsetAsync(nan_flag.p, 0, sizeof(int), m.stream));
    FR_HIP(hipMemsetAsync(h.edges.p, 0, F * HIST_MAX_BINS * sizeof(float), m.stream));
    size_t temp_bytes = 0;
    FR_HIP(rocprim::radix_sort_keys(nullptr, temp_bytes, col.p, sorted.p, n, 0u, 32u, m.stream));
    if (!h.temp.ensure(std::max<size_t>(temp_bytes, 16), err)) return false;
    const uint32_t n32 = (uint32_t)n;
    {
        ProfScope ps("hist_binning", m.stream);
        for (size_t s = 0; s < F; s++) {
            hist_column_kernel<<<grid1d(n, 256), 256, 0, m.stream>>>(m.xb.p, (uint32_t)m.dq, h.pos.p, n32, feats[s], col.p, nan_flag.p);
            size_t tb = h.temp.bytes();
            FR_HIP(rocprim::radix_sort_keys((void*)h.temp.p, tb, col.p, sorted.p, n, 0u, 32u, m.stream));
            hist_distinct_kernel<<<grid1d(n, 256), 256, 0, m.stream>>>(sorted.p, n32, count.p + s, firsts.p + s * (HIST_MAX_BINS + 1));
            hist_edges_kernel<<<1, 256, 0, m.stream>>>(sorted.p, n32, k, count.p + s, firsts.p + s * (HIST_MAX_BINS + 1),
                                                       h.edges.p + s * HIST_MAX_BINS, h.nedges.p + s);
            hist_bin_kernel<<<grid1d(n, 256), 256, 0, m.stream>>>(col.p, n32, h.edges.p + s * HIST_MAX_BINS, h.nedges.p + s, h.xbin.p + s * n);
        }
    }
    FR_HIP(hipGetLastError());
    h.edges_host.assign(F * HIST_MAX_BINS, 0.0f);
    h.nedges_host.assign(F, 0);
    int bad = 0;
    FR_HIP(hipMemcpyAsync(h.edges_host.data(), h.edges.p, F * HIST_MAX_BINS * sizeof(float), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(h.nedges_host.data(), h.nedges.p, F * sizeof(uint32_t), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(&bad, nan_flag.p, sizeof(int), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    if (bad) return hist_fail(err, "a feature value is NaN; NaN has no bin (use the exact grower, or clean the data)");
    for (size_t s = 0; s < F; s++)
        if (h.nedges_host[s] >= k) return hist_fail(err, "internal error: more edges than bins");
    h.qof_built = false;  // (made for these bins by the first query sample: hist_qof)
    h.mono_F = 0;
    h.feats = feats;
    h.n = n32, h.F = (uint32_t)F, h.k = k;
    h.nt = n32, h.Ft = (uint32_t)F, h.q_sampled = h.f_sampled = h.g_on = h.qz_on = false;
    if (built) *built = true;
    return true;
}

bool DeviceDataset::hist_edges(std::vector<float>* edges, std::vector<uint32_t>* nedges, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (m.hist.k == 0) return hist_fail(err, "no bins built");
    *edges = m.hist.edges_host;
    *nedges = m.hist.nedges_host;
    return true;
}

bool DeviceDataset::hist_download_bins(uint8_t* out, size_t len, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    if (h.k == 0) return hist_fail(err, "no bins built");
    if (len != (size_t)h.F * h.n) return hist_fail(err, "bin matrix output has the wrong length");
    FR_HIP(hipMemcpyAsync(out, h.xbin.p, len, hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    return true;
}

// the query of every instance-list entry, for the trees' query samples: made once per bin matrix, by the first tree that
// samples queries (4 ms of host work at the 30K shape that a request without samples does not pay)
bool DeviceDataset::Impl::hist_qof(std::string* err) {
    auto& h = hist;
    if (h.qof_built) return true;
    std::vector<uint32_t> q_of_pos(np, IDX_INVALID), qof(h.n);
    for (size_t q = 0; q < nq; q++)
        for (uint32_t j = 0; j < qlen_h[q]; j++) q_of_pos[qstart_h[q] + j] = (uint32_t)q;
    h.qof_ok = true;
    for (size_t i = 0; i < h.n; i++) {
        qof[i] = q_of_pos[h.pos_host[i]];
        if (qof[i] == IDX_INVALID) h.qof_ok = false, qof[i] = 0;
    }
    if (!upload(h.qof, qof, err)) return false;
    h.qof_built = true;
    return true;
}

bool DeviceDataset::Impl::hist_flag_scan(uint32_t begin, uint32_t count, std::string* err) {
    auto& h = hist;
    size_t tb = 0;
    FR_HIP(rocprim::exclusive_scan(nullptr, tb, h.flag.p + begin, h.scan.p + begin, 0u, (size_t)count, rocprim::plus<uint32_t>(), stream));
    if (tb > h.temp.bytes()) {
        FR_HIP(hipStreamSynchronize(stream));  // (no earlier user of the scratch -- binning's sort, an earlier scan -- is in flight)
        if (!h.temp.ensure(tb, err)) return false;
    }
    FR_HIP(rocprim::exclusive_scan((void*)h.temp.p, tb, h.flag.p + begin, h.scan.p + begin, 0u, (size_t)count, rocprim::plus<uint32_t>(), stream));
    return true;
}

bool DeviceDataset::hist_sample(const unsigned char* query_flags, uint32_t n_t, const uint32_t* fsel, size_t f_t, std::string* err,
                                bool keep_queries) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    if (h.k == 0) return hist_fail(err, "no bins built");
    const uint32_t n = h.n;
    h.g_on = h.qz_on = false;  // (GOSS and the quantised gradients are a tree's: hist_goss / hist_quantq set them after the sample)
    if (keep_queries && query_flags == nullptr && h.q_sampled) {  // (the root list and its length stay)
        n_t = h.nt;
        h.Ft = h.F, h.f_sampled = false;
    } else {
        h.nt = n, h.Ft = h.F, h.q_sampled = h.f_sampled = false;
    }
    if (fsel != nullptr) {
        if (f_t == 0 || f_t > h.F) return hist_fail(err, "a feature sample must hold between 1 and all of the features");
        for (size_t i = 0; i < f_t; i++)
            if (fsel[i] >= h.F || (i > 0 && fsel[i] <= fsel[i - 1])) return hist_fail(err, "a feature sample must be ascending slots of the bin matrix");
        if (!h.fsel.ensure(h.F, err)) return false;
        FR_HIP(hipMemcpyAsync(h.fsel.p, fsel, f_t * sizeof(uint32_t), hipMemcpyHostToDevice, m.stream));
    }
    uint32_t total = n_t;
    if (query_flags != nullptr) {
        if (!m.hist_qof(err)) return false;
        if (!h.qof_ok) return hist_fail(err, "an instance of the list belongs to no query of the dataset: no query sample");
        if (n_t == 0 || n_t > n) return hist_fail(err, "a query sample must hold between 1 and all of the instances");
        if (!h.qflag.ensure(m.nq, err) || !h.root.ensure(n, err) || !h.flag.ensure(n, err) || !h.scan.ensure(n, err) || !h.total.ensure(1, err))
            return false;
        FR_HIP(hipMemcpyAsync(h.qflag.p, query_flags, m.nq, hipMemcpyHostToDevice, m.stream));
        ProfScope ps("hist_rootlist", m.stream);
        hist_qflag_kernel<<<grid1d(n, 256), 256, 0, m.stream>>>(h.qof.p, h.qflag.p, n, h.flag.p);
        if (!m.hist_flag_scan(0, n, err)) return false;
        hist_rootlist_kernel<<<grid1d(n, 256), 256, 0, m.stream>>>(h.flag.p, h.scan.p, n, n_t, h.root.p, h.total.p);
        FR_HIP(hipGetLastError());
        FR_HIP(hipMemcpyAsync(&total, h.total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, m.stream));
    }
    FR_HIP(hipStreamSynchronize(m.stream));  // (query_flags / fsel are the caller's pageable memory)
    if (total != n_t) return hist_fail(err, "internal error: the query sample holds " + std::to_string(total) + " instances, not " + std::to_string(n_t));
    if (query_flags != nullptr) h.nt = n_t, h.q_sampled = true;
    if (fsel != nullptr) h.Ft = (uint32_t)f_t, h.f_sampled = true;
    return true;
}

bool DeviceDataset::hist_quantise(const double* lam_list, const double* wt_list, int* s_l, int* s_w, bool* all_zero, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    if (h.k == 0) return hist_fail(err, "no bins built");
    h.qz_on = false;  // (a tree's: hist_quantq sets it after this)
    const uint32_t n = h.n, nt = h.tree_n();  // (host arrays and Q / W: the full list; the maxima, c and the quantisation: the tree's)
    const double *lam = nullptr, *wt = nullptr;
    const uint32_t *pos = nullptr, *root = h.tree_root();
    if (lam_list != nullptr) {
        if (!h.lam_in.ensure(n, err) || !h.wt_in.ensure(n, err)) return false;
        FR_HIP(hipMemcpyAsync(h.lam_in.p, lam_list, n * sizeof(double), hipMemcpyHostToDevice, m.stream));
        FR_HIP(hipMemcpyAsync(h.wt_in.p, wt_list, n * sizeof(double), hipMemcpyHostToDevice, m.stream));
        lam = h.lam_in.p, wt = h.wt_in.p;
    } else {
        if (!m.lm.built) return hist_fail(err, "no gradients computed");
        lam = m.lm.lam.p, wt = m.lm.wt.p, pos = h.pos.p;
    }
    if (!h.absmax.ensure(2, err) || !h.Q.ensure(n, err) || !h.W.ensure(n, err)) return false;
    FR_HIP(hipMemsetAsync(h.absmax.p, 0, 2 * sizeof(unsigned long long), m.stream));
    if (h.g_on) {  // (the kept others amplified before the maximum: kernels_goss.inc)
        ProfScope ps("goss_absmax_kernel", m.stream);
        goss_absmax_kernel<<<std::min<unsigned>(grid1d(nt, 256).x, 1024u), 256, 0, m.stream>>>(lam, wt, pos, root, h.gtop.p, h.g_amp, nt, h.absmax.p);
    } else {
        ProfScope ps("hist_absmax_kernel", m.stream);
        hist_absmax_kernel<<<std::min<unsigned>(grid1d(nt, 256).x, 1024u), 256, 0, m.stream>>>(lam, wt, pos, root, nt, h.absmax.p);
    }
    unsigned long long bits[2] = {0, 0};
    FR_HIP(hipMemcpyAsync(bits, h.absmax.p, sizeof(bits), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    double mx[2];
    std::memcpy(mx, bits, sizeof(mx));
    if (!std::isfinite(mx[0]) || !std::isfinite(mx[1])) return hist_fail(err, "a gradient is not finite");
    *all_zero = mx[0] == 0.0;
    *s_l = *s_w = 0;
    if (*all_zero) return true;
    uint32_t c = 0;  // ceil(log2(n + 1)) = the bit length of n
    for (uint32_t x = nt; x != 0; x >>= 1) c++;
    int e = 0;
    (void)std::frexp(mx[0], &e);
    *s_l = 61 - e - (int)c;
    if (mx[1] != 0.0) {
        (void)std::frexp(mx[1], &e);
        *s_w = 61 - e - (int)c;
    }
    if (h.g_on) {
        ProfScope ps("goss_quant_kernel", m.stream);
        goss_quant_kernel<<<grid1d(nt, 256), 256, 0, m.stream>>>(lam, wt, pos, root, h.gtop.p, h.g_amp, nt, *s_l, *s_w, mx[1] == 0.0 ? 1 : 0, h.Q.p, h.W.p);
    } else {
        ProfScope ps("hist_quant_kernel", m.stream);
        hist_quant_kernel<<<grid1d(nt, 256), 256, 0, m.stream>>>(lam, wt, pos, root, nt, *s_l, *s_w, mx[1] == 0.0 ? 1 : 0, h.Q.p, h.W.p);
    }
    FR_HIP(hipGetLastError());
    return true;
}

// Quantised gradients (kernels_histquant.inc): one launch over the tree's list; waited for, so that quant_ms is its time
bool DeviceDataset::hist_quantq(uint32_t bits, uint64_t tree_key, int* d, int* d_w, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    if (h.k == 0) return hist_fail(err, "no bins built");
    h.qz_on = false;
    if (bits < fr::QUANT_MIN_BITS || bits > fr::QUANT_MAX_BITS) return hist_fail(err, "internal error: grad_quant_bits outside 2..8");
    const uint32_t nt = h.tree_n();
    if (nt == 0 || h.Q.cap < h.n || h.W.cap < h.n) return hist_fail(err, "internal error: no fixed-point gradients to quantise");
    const fr::QuantShifts sh = fr::quant_shifts(nt, bits);
    if (sh.d < 1 || sh.d > 63 || sh.d_w < 1 || sh.d_w > 63) return hist_fail(err, "internal error: a quantisation shift outside 1..63");
    if (!h.packed.ensure(h.n, err)) return false;
    {
        ProfScope ps("hist_quantq_kernel", m.stream);
        hist_quantq_kernel<<<grid1d(nt, 256), 256, 0, m.stream>>>(h.Q.p, h.W.p, h.tree_root(), h.pos.p, m.perm.p, nt, tree_key, sh.d, sh.d_w, h.packed.p);
    }
    FR_HIP(hipGetLastError());
    FR_HIP(hipStreamSynchronize(m.stream));
    *d = sh.d, *d_w = sh.d_w;
    h.qz_on = true;
    return true;
}

bool DeviceDataset::hist_quantq_download(int32_t* q, uint32_t* w, size_t len, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    if (!h.qz_on || len != h.tree_n()) return hist_fail(err, "no quantised gradients of that length");
    std::vector<uint32_t> by_index(h.n), list(h.tree_root() != nullptr ? len : 0);
    FR_HIP(hipMemcpyAsync(by_index.data(), h.packed.p, (size_t)h.n * sizeof(uint32_t), hipMemcpyDeviceToHost, m.stream));
    if (!list.empty()) FR_HIP(hipMemcpyAsync(list.data(), h.tree_root(), len * sizeof(uint32_t), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    for (size_t i = 0; i < len; i++) {
        const uint32_t p = by_index[list.empty() ? i : list[i]];
        q[i] = fr::quant_unpack_q(p), w[i] = fr::quant_unpack_w(p);
    }
    return true;
}

bool DeviceDataset::hist_root_download(uint32_t* cnt, long long* sum, long long* wsum, size_t cells, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    if (h.k == 0 || cells != (size_t)h.Ft * h.k || h.cnt.cap < cells || h.sum.cap < cells || h.wsum.cap < cells)
        return hist_fail(err, "no root histogram of that size");
    FR_HIP(hipMemcpyAsync(cnt, h.cnt.p, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(sum, h.sum.p, cells * sizeof(long long), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(wsum, h.wsum.p, cells * sizeof(long long), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    return true;
}

// GOSS (kernels_goss.inc): select chain, the two flag stages, the list.  One wait at the end, for the list's length.
bool DeviceDataset::hist_goss(const double* lam_list, uint32_t n_top, double p, double amp, uint64_t tree_key, uint32_t* n_g, uint64_t* tau,
                              std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    if (h.k == 0) return hist_fail(err, "no bins built");
    h.g_on = false;
    const uint32_t n = h.n, nt = h.nt;
    const uint32_t* root = h.q_sampled ? h.root.p : nullptr;
    if (nt == 0 || n_top == 0 || n_top > nt) return hist_fail(err, "internal error: GOSS needs between 1 and all of the tree's instances in the top set");
    if (!(p > 0.0) || !std::isfinite(p) || !(amp > 0.0) || !std::isfinite(amp)) return hist_fail(err, "internal error: GOSS rates outside their range");
    const double* lam = nullptr;
    const uint32_t* pos = nullptr;
    if (lam_list != nullptr) {
        if (!h.lam_in.ensure(n, err)) return false;
        FR_HIP(hipMemcpyAsync(h.lam_in.p, lam_list, n * sizeof(double), hipMemcpyHostToDevice, m.stream));
        lam = h.lam_in.p;
    } else {
        if (!m.lm.built) return hist_fail(err, "no gradients computed");
        lam = m.lm.lam.p, pos = h.pos.p;
    }
    if (!h.gkeys.ensure(n, err) || !h.ghist.ensure((size_t)GOSS_PASSES * GOSS_BINS, err) || !h.gstate.ensure(1, err) || !h.gtop.ensure(n, err) ||
        !h.groot.ensure(n, err) || !h.flag.ensure(n, err) || !h.scan.ensure(n, err) || !h.total.ensure(1, err))
        return false;
    FR_HIP(hipMemsetAsync(h.ghist.p, 0, (size_t)GOSS_PASSES * GOSS_BINS * sizeof(uint32_t), m.stream));
    {
        ProfScope ps("goss_select", m.stream);
        const unsigned g = (nt + GOSS_SHARE - 1) / GOSS_SHARE;
        for (uint32_t pass = 0; pass < GOSS_PASSES; pass++) {
            if (pass == 0) goss_hist_kernel<true><<<g, 256, 0, m.stream>>>(lam, pos, root, nt, pass, h.gstate.p, h.gkeys.p, h.ghist.p);
            else goss_hist_kernel<false><<<g, 256, 0, m.stream>>>(lam, pos, root, nt, pass, h.gstate.p, h.gkeys.p, h.ghist.p);
            goss_pick_kernel<<<1, 64, 0, m.stream>>>(h.ghist.p, pass, n_top, h.gstate.p);
        }
        FR_HIP(hipGetLastError());
    }
    uint32_t total = 0;
    GossStateDev st{};
    {
        ProfScope ps("goss_flag", m.stream);
        if (root != nullptr) FR_HIP(hipMemsetAsync(h.flag.p, 0, n * sizeof(uint32_t), m.stream));  // (entries outside the list: never kept)
        goss_tie_kernel<<<grid1d(nt, 256), 256, 0, m.stream>>>(h.gkeys.p, root, nt, h.gstate.p, h.flag.p);
        if (!m.hist_flag_scan(0, n, err)) return false;
        goss_flag_kernel<<<grid1d(nt, 256), 256, 0, m.stream>>>(h.gkeys.p, root, nt, h.gstate.p, h.scan.p, h.pos.p, m.perm.p, tree_key, p, h.gtop.p, h.flag.p);
        if (!m.hist_flag_scan(0, n, err)) return false;
        hist_rootlist_kernel<<<grid1d(n, 256), 256, 0, m.stream>>>(h.flag.p, h.scan.p, n, nt, h.groot.p, h.total.p);
        FR_HIP(hipGetLastError());
        FR_HIP(hipMemcpyAsync(&total, h.total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, m.stream));
        if (tau != nullptr) FR_HIP(hipMemcpyAsync(&st, h.gstate.p, sizeof(st), hipMemcpyDeviceToHost, m.stream));
    }
    FR_HIP(hipStreamSynchronize(m.stream));  // (lam_list is the caller's pageable memory as well)
    if (total < n_top || total > nt)
        return hist_fail(err, "internal error: the GOSS list holds " + std::to_string(total) + " instances for a top set of " + std::to_string(n_top));
    if (tau != nullptr) *tau = st.prefix;
    *n_g = total;
    h.g_on = true, h.ng = total, h.g_amp = amp;
    return true;
}

bool DeviceDataset::hist_goss_download(uint32_t* list, uint8_t* top, size_t len, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    if (!h.g_on || len != h.ng) return hist_fail(err, "no GOSS list of that length");
    std::vector<uint8_t> by_index(h.n);
    FR_HIP(hipMemcpyAsync(list, h.groot.p, len * sizeof(uint32_t), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(by_index.data(), h.gtop.p, h.n, hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    for (size_t i = 0; i < len; i++) top[i] = by_index[list[i]];
    return true;
}

// the stretches cut into pieces of at most HIST_CHUNK entries (slot carried along): one workgroup each
bool DeviceDataset::Impl::hist_items(const std::vector<HistItemDev>& stretches, std::vector<HistItemDev>& host, DevBuf<HistItemDev>& dev,
                                     std::string* err) {
    host.clear();
    for (const HistItemDev& s : stretches)
        for (uint32_t b = s.begin; b < s.end; b += HIST_CHUNK) host.push_back({s.slot, b, std::min(s.end, b + HIST_CHUNK)});
    if (host.empty()) return true;
    if (!dev.ensure(host.size(), err)) return false;
    FR_HIP(hipMemcpyAsync(dev.p, host.data(), host.size() * sizeof(HistItemDev), hipMemcpyHostToDevice, stream));
    return true;
}

void DeviceDataset::Impl::hist_build(uint32_t* cnt, unsigned long long* sum, unsigned long long* wsum) {
    auto& h = hist;
    const uint32_t* fsel = h.f_sampled ? h.fsel.p : nullptr;
    if (wsum == nullptr) {
        ProfScope ps("hist_build_kernel", stream);
        const dim3 grid((unsigned)h.items_bh.size(), (h.Ft + HIST_FB - 1) / HIST_FB);
        const size_t lds = (size_t)HIST_FB * h.k * 12;
        if (h.f_sampled)
            hist_build_kernel<true><<<grid, 256, lds, stream>>>(h.items_b.p, h.xbin.p, h.n, h.idx.p, h.Q.p, fsel, h.Ft, h.k, cnt, sum);
        else
            hist_build_kernel<false><<<grid, 256, lds, stream>>>(h.items_b.p, h.xbin.p, h.n, h.idx.p, h.Q.p, fsel, h.Ft, h.k, cnt, sum);
    } else if (h.qz_on) {  // (quantised gradients: the packed values instead of Q / W, the same three arrays out)
        ProfScope ps("hist_build_packed_kernel", stream);
        const dim3 grid((unsigned)h.items_bh.size(), (h.Ft + HIST_FB_PACKED - 1) / HIST_FB_PACKED);
        const size_t lds = (size_t)HIST_FB_PACKED * h.k * 8;
        if (h.f_sampled)
            hist_build_packed_kernel<true><<<grid, 256, lds, stream>>>(h.items_b.p, h.xbin.p, h.n, h.idx.p, h.packed.p, fsel, h.Ft, h.k, cnt, sum, wsum);
        else
            hist_build_packed_kernel<false><<<grid, 256, lds, stream>>>(h.items_b.p, h.xbin.p, h.n, h.idx.p, h.packed.p, fsel, h.Ft, h.k, cnt, sum, wsum);
    } else {
        ProfScope ps("hist_build_newton_kernel", stream);
        const dim3 grid((unsigned)h.items_bh.size(), (h.Ft + HIST_FB_NEWTON - 1) / HIST_FB_NEWTON);
        const size_t lds = (size_t)HIST_FB_NEWTON * h.k * 20;
        if (h.f_sampled)
            hist_build_newton_kernel<true><<<grid, 256, lds, stream>>>(h.items_b.p, h.xbin.p, h.n, h.idx.p, h.Q.p, h.W.p, fsel, h.Ft, h.k, cnt, sum, wsum);
        else
            hist_build_newton_kernel<false><<<grid, 256, lds, stream>>>(h.items_b.p, h.xbin.p, h.n, h.idx.p, h.Q.p, h.W.p, fsel, h.Ft, h.k, cnt, sum, wsum);
    }
}

// zeroes `cells` cells from cell `off` on of the histograms
bool DeviceDataset::Impl::hist_zero(uint32_t* cnt, unsigned long long* sum, unsigned long long* wsum, size_t off, size_t cells, std::string* err) {
    FR_HIP(hipMemsetAsync(cnt + off, 0, cells * sizeof(uint32_t), stream));
    FR_HIP(hipMemsetAsync(sum + off, 0, cells * sizeof(unsigned long long), stream));
    if (wsum != nullptr) FR_HIP(hipMemsetAsync(wsum + off, 0, cells * sizeof(unsigned long long), stream));
    return true;
}

// the nodes of a search into hist.nodes (their staging: hist.nodes_h), each held to the level's histograms (to the Newton
// gain's third array too when `newton`) and to the index list
bool DeviceDataset::Impl::hist_stage_nodes(const std::vector<DeviceDataset::HistNode>& nodes, bool newton, std::string* err) {
    static_assert(sizeof(DeviceDataset::HistNode) == sizeof(HistItemDev), "host and device records differ");
    auto& h = hist;
    const size_t A = nodes.size(), fk = (size_t)h.Ft * h.k;
    h.nodes_h.resize(A);
    for (size_t a = 0; a < A; a++) {
        const size_t cells = (size_t)(nodes[a].slot + 1) * fk;
        if (cells > h.cnt.cap || (newton && cells > h.wsum.cap) || nodes[a].end > h.tree_n() || nodes[a].begin > nodes[a].end)
            return hist_fail(err, "internal error: a node outside the level's histograms");
        h.nodes_h[a] = {nodes[a].slot, nodes[a].begin, nodes[a].end};
    }
    if (!h.nodes.ensure(A, err)) return false;
    FR_HIP(hipMemcpyAsync(h.nodes.p, h.nodes_h.data(), A * sizeof(HistItemDev), hipMemcpyHostToDevice, stream));
    return true;
}

// a search's records back to the host; waits for the stream
template <typename Host, typename Dev>
static bool hist_fetch(std::vector<Host>* out, const DevBuf<Dev>& dev, hipStream_t stream, std::string* err) {
    static_assert(sizeof(Host) == sizeof(Dev), "host and device records differ");
    FR_HIP(hipMemcpyAsync(out->data(), dev.p, out->size() * sizeof(Dev), hipMemcpyDeviceToHost, stream));
    FR_HIP(hipStreamSynchronize(stream));
    return true;
}

// a level's arrays (under the Newton gain its third one too): a plain error when they do not fit
static bool hist_level_alloc(DevBuf<uint32_t>& cnt, DevBuf<unsigned long long>& sum, DevBuf<unsigned long long>& wsum, size_t cells, bool newton,
                             std::string* err) {
    std::string e2;
    if (!cnt.ensure(cells, &e2) || !sum.ensure(cells, &e2)) {
        (void)hipGetLastError();
        return hist_fail(err, "no device memory for a level's histograms (" + std::to_string((cells * 12) >> 20) +
                                  " MB: open nodes x features x bins x 12 bytes); lower max_depth or split_candidates");
    }
    if (newton && !wsum.ensure(cells, &e2)) {
        (void)hipGetLastError();
        return hist_fail(err, "no device memory for a level's histograms (" + std::to_string((cells * 20) >> 20) +
                                  " MB: open nodes x features x bins x 20 bytes under the Newton gain); lower max_depth or split_candidates");
    }
    return true;
}

// The root of a tree: the index list (a copy of the tree's root list, or 0..n-1), the one root item, and the root's histogram
// zeroed and built into cell 0 on of the given arrays
bool DeviceDataset::Impl::hist_root_build(uint32_t* cnt, unsigned long long* sum, unsigned long long* wsum, std::string* err) {
    auto& h = hist;
    const uint32_t n = h.tree_n();  // the tree's instances: the index list's length (the bin matrix's rows hold h.n)
    if (!hist_zero(cnt, sum, wsum, 0, (size_t)h.Ft * h.k, err)) return false;
    if (h.tree_root() != nullptr) {
        FR_HIP(hipMemcpyAsync(h.idx.p, h.tree_root(), n * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    } else {
        hist_iota_kernel<<<grid1d(n, 256), 256, 0, stream>>>(h.idx.p, n);
    }
    if (!hist_items({{0u, 0u, n}}, h.items_bh, h.items_b, err)) return false;
    hist_build(cnt, sum, wsum);
    FR_HIP(hipGetLastError());
    return true;
}

bool DeviceDataset::hist_root(bool newton, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    if (h.k == 0) return hist_fail(err, "no bins built");
    if (!h.idx.ensure(h.n, err) || !h.idx_o.ensure(h.n, err) || !h.flag.ensure(h.n, err) || !h.scan.ensure(h.n, err)) return false;
    if (!hist_level_alloc(h.cnt, h.sum, h.wsum, (size_t)h.Ft * h.k, newton, err)) return false;
    FR_HIP(hipMemsetAsync(h.flag.p, 0, h.tree_n() * sizeof(uint32_t), m.stream));
    return m.hist_root_build(h.cnt.p, h.sum.p, newton ? h.wsum.p : nullptr, err);
}

// the numbers of a regularised search as its kernels take them
static HistRegDev hist_reg_numbers(const DeviceDataset::HistSearch& how) {
    return {how.lambda_l1, how.lambda_l2, how.max_delta_step, how.path_smooth, how.min_sum_hessian};
}

bool DeviceDataset::hist_search(const std::vector<HistNode>& nodes, const HistSearch& how, const std::vector<HistBounds>* bounds,
                                std::vector<HistCand>* best, std::string* err, const std::vector<HistRegNode>* reg) {
    static_assert(sizeof(HistBounds) == sizeof(HistBoundsDev), "host and device records differ");
    static_assert(sizeof(HistRegNode) == sizeof(HistRegNodeDev), "host and device records differ");
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    const size_t A = nodes.size();
    best->assign(A * h.Ft, HistCand{});
    if (A == 0) return true;
    if (how.reg()) {
        if (!how.newton || reg == nullptr || reg->size() != A) return hist_fail(err, "internal error: one regularisation record per node is needed");
        if (h.mono_F == 0 || h.mono_F != h.F) return hist_fail(err, "internal error: no monotone signs set for these bins");
    } else if (how.monotone) {
        if (!how.newton || bounds == nullptr || bounds->size() != A) return hist_fail(err, "internal error: one interval per node is needed");
        if (h.mono_F == 0 || h.mono_F != h.F) return hist_fail(err, "internal error: no monotone signs set for these bins");
    }
    if (!m.hist_stage_nodes(nodes, how.newton, err)) return false;
    const unsigned grid = (unsigned)(A * h.Ft);
    const uint32_t* fsel = h.f_sampled ? h.fsel.p : nullptr;
    if (!how.newton) {  // the variance criterion's shorter record, widened: wl = wtot = 0
        if (!h.best.ensure(A * h.Ft, err)) return false;
        {
            ProfScope ps("hist_scan_kernel", m.stream);
            hist_scan_kernel<<<grid, 64, 0, m.stream>>>(h.nodes.p, h.Ft, h.k, h.nedges.p, fsel, h.cnt.p, h.sum.p, how.min_leaf, h.best.p);
        }
        FR_HIP(hipGetLastError());
        h.best_h.resize(A * h.Ft);
        if (!hist_fetch(&h.best_h, h.best, m.stream, err)) return false;
        for (size_t i = 0; i < h.best_h.size(); i++) {
            const HistBestDev& b = h.best_h[i];
            (*best)[i] = {b.imp, b.ql, b.qtot, 0ll, 0ll, b.edge, b.nl, b.valid, 0u};
        }
        return true;
    }
    if (!h.best_n.ensure(A * h.Ft, err)) return false;
    if (how.reg()) {
        if (!h.regn.ensure(A, err)) return false;
        FR_HIP(hipMemcpyAsync(h.regn.p, reg->data(), A * sizeof(HistRegNodeDev), hipMemcpyHostToDevice, m.stream));
        ProfScope ps("hist_scan_reg_kernel", m.stream);
        hist_scan_reg_kernel<<<grid, 64, 0, m.stream>>>(h.nodes.p, h.regn.p, h.Ft, h.k, h.nedges.p, h.mono.p, fsel, h.cnt.p, h.sum.p, h.wsum.p, how.min_leaf,
                                                        how.s_l, how.s_w, hist_reg_numbers(how), h.best_n.p);
    } else if (how.monotone) {
        if (!h.bounds.ensure(A, err)) return false;
        FR_HIP(hipMemcpyAsync(h.bounds.p, bounds->data(), A * sizeof(HistBoundsDev), hipMemcpyHostToDevice, m.stream));
        ProfScope ps("hist_scan_monotone_kernel", m.stream);
        hist_scan_monotone_kernel<<<grid, 64, 0, m.stream>>>(h.nodes.p, h.bounds.p, h.Ft, h.k, h.nedges.p, h.mono.p, fsel, h.cnt.p, h.sum.p, h.wsum.p,
                                                             how.min_leaf, how.s_l, how.s_w, how.lambda_l2, how.min_sum_hessian, h.best_n.p);
    } else {
        ProfScope ps("hist_scan_newton_kernel", m.stream);
        hist_scan_newton_kernel<<<grid, 64, 0, m.stream>>>(h.nodes.p, h.Ft, h.k, h.nedges.p, fsel, h.cnt.p, h.sum.p, h.wsum.p, how.min_leaf, how.s_l,
                                                           how.s_w, how.lambda_l2, how.min_sum_hessian, h.best_n.p);
    }
    FR_HIP(hipGetLastError());
    return hist_fetch(best, h.best_n, m.stream, err);  // (*bounds / *reg is the caller's, read by the copy above until this has waited)
}

bool DeviceDataset::hist_monotone(const int* signs, size_t features, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    if (h.k == 0) return hist_fail(err, "no bins built");
    if (signs == nullptr || features != h.F) return hist_fail(err, "internal error: the monotone signs do not cover the bin matrix's rows");
    for (size_t i = 0; i < features; i++)
        if (signs[i] < -1 || signs[i] > 1) return hist_fail(err, "internal error: a monotone sign outside {-1, 0, 1}");
    h.mono_F = 0;
    if (!h.mono.ensure(features, err)) return false;
    FR_HIP(hipMemcpyAsync(h.mono.p, signs, features * sizeof(int), hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));  // (signs is the caller's pageable memory)
    h.mono_F = (uint32_t)features;
    return true;
}

bool DeviceDataset::hist_search_symmetric(const std::vector<HistNode>& nodes, const HistSearch& how, std::vector<HistSymBest>* best,
                                          std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    const size_t A = nodes.size();
    best->assign(h.Ft, HistSymBest{});
    if (A == 0 || h.Ft == 0) return true;
    if (h.k < 2 || h.k > HIST_MAX_BINS) return hist_fail(err, "internal error: no bins built");
    if (how.reg() && (!how.newton || how.path_smooth != 0.0)) return hist_fail(err, "internal error: a symmetric level takes lambda_l1 and max_delta_step under the Newton gain only");
    if (!m.hist_stage_nodes(nodes, how.newton, err) || !h.best_sym.ensure(h.Ft, err)) return false;
    const uint32_t* fsel = h.f_sampled ? h.fsel.p : nullptr;
    {
        ProfScope ps(how.reg() ? "hist_scan_sym_reg_kernel" : "hist_scan_sym_kernel", m.stream);
        if (how.reg())
            hist_scan_sym_reg_kernel<<<h.Ft, 256, 0, m.stream>>>(h.nodes.p, (uint32_t)A, h.Ft, h.k, h.nedges.p, fsel, h.cnt.p, h.sum.p, h.wsum.p,
                                                                 how.min_leaf, how.s_l, how.s_w, hist_reg_numbers(how), how.min_split_gain,
                                                                 h.best_sym.p);
        else if (how.newton)
            hist_scan_sym_kernel<true><<<h.Ft, 256, 0, m.stream>>>(h.nodes.p, (uint32_t)A, h.Ft, h.k, h.nedges.p, fsel, h.cnt.p, h.sum.p, h.wsum.p,
                                                                   how.min_leaf, how.s_l, how.s_w, how.lambda_l2, how.min_sum_hessian,
                                                                   how.min_split_gain, h.best_sym.p);
        else
            hist_scan_sym_kernel<false><<<h.Ft, 256, 0, m.stream>>>(h.nodes.p, (uint32_t)A, h.Ft, h.k, h.nedges.p, fsel, h.cnt.p, h.sum.p, nullptr,
                                                                    how.min_leaf, 0, 0, 0.0, 0.0, 0.0, h.best_sym.p);
    }
    FR_HIP(hipGetLastError());
    return hist_fetch(best, h.best_sym, m.stream, err);
}

bool DeviceDataset::hist_symmetric_apply(const std::vector<HistNode>& nodes, const HistSearch& how, uint32_t fi, uint32_t edge,
                                         std::vector<HistCand>* out, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    const size_t A = nodes.size();
    out->assign(A, HistCand{});
    if (A == 0) return true;
    if (h.k < 2 || h.k > HIST_MAX_BINS || fi >= h.Ft || edge + 1 >= h.k) return hist_fail(err, "internal error: a level's split outside the histograms");
    if (how.reg() && (!how.newton || how.path_smooth != 0.0)) return hist_fail(err, "internal error: a symmetric level takes lambda_l1 and max_delta_step under the Newton gain only");
    // (the level's search has staged these very nodes, and has waited for the stream: they are uploaded again only if they differ)
    static_assert(sizeof(HistNode) == sizeof(HistItemDev), "host and device records differ");
    const bool staged = h.nodes_h.size() == A && std::memcmp(h.nodes_h.data(), nodes.data(), A * sizeof(HistItemDev)) == 0;
    if ((!staged && !m.hist_stage_nodes(nodes, how.newton, err)) || !h.best_n.ensure(A, err)) return false;
    {
        ProfScope ps(how.reg() ? "hist_sym_apply_reg_kernel" : "hist_sym_apply_kernel", m.stream);
        if (how.reg())
            hist_sym_apply_reg_kernel<<<(unsigned)A, 64, 0, m.stream>>>(h.nodes.p, h.Ft, h.k, fi, edge, h.cnt.p, h.sum.p, h.wsum.p, how.min_leaf, how.s_l,
                                                                        how.s_w, hist_reg_numbers(how), how.min_split_gain, h.best_n.p);
        else if (how.newton)
            hist_sym_apply_kernel<true><<<(unsigned)A, 64, 0, m.stream>>>(h.nodes.p, h.Ft, h.k, fi, edge, h.cnt.p, h.sum.p, h.wsum.p, how.min_leaf,
                                                                          how.s_l, how.s_w, how.lambda_l2, how.min_sum_hessian, how.min_split_gain,
                                                                          h.best_n.p);
        else
            hist_sym_apply_kernel<false><<<(unsigned)A, 64, 0, m.stream>>>(h.nodes.p, h.Ft, h.k, fi, edge, h.cnt.p, h.sum.p, nullptr, how.min_leaf, 0, 0,
                                                                           0.0, 0.0, 0.0, h.best_n.p);
    }
    FR_HIP(hipGetLastError());
    return hist_fetch(out, h.best_n, m.stream, err);
}

bool DeviceDataset::hist_split(const std::vector<HistSplit>& splits, const std::vector<HistNode>& builds, const std::vector<HistSub>& subs,
                               uint32_t next_slots, bool newton, std::string* err) {
    static_assert(sizeof(HistSplit) == sizeof(HistSplitDev) && sizeof(HistSub) == sizeof(HistSubDev), "host and device records differ");
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    const uint32_t n = h.tree_n();  // the index list's length; the bin matrix's rows hold h.n entries
    const size_t fk = (size_t)h.Ft * h.k;
    if (!splits.empty()) {
        std::vector<HistItemDev> stretches(splits.size());
        h.splits_h.resize(splits.size());
        for (size_t i = 0; i < splits.size(); i++) {
            const HistSplit& s = splits[i];
            if (s.begin >= s.end || s.end > n || s.nl > s.end - s.begin || s.fslot >= h.F || s.edge >= h.k)
                return hist_fail(err, "internal error: a split outside the index list");
            h.splits_h[i] = {s.begin, s.end, s.fslot, s.edge, s.nl};
            stretches[i] = {(uint32_t)i, s.begin, s.end};
        }
        if (!h.splits.ensure(splits.size(), err) || !m.hist_items(stretches, h.items_h, h.items, err)) return false;
        FR_HIP(hipMemcpyAsync(h.splits.p, h.splits_h.data(), splits.size() * sizeof(HistSplitDev), hipMemcpyHostToDevice, m.stream));
        const unsigned g = (unsigned)h.items_h.size();
        ProfScope ps("hist_partition", m.stream);
        hist_flag_kernel<<<g, 256, 0, m.stream>>>(h.items.p, h.splits.p, h.xbin.p, h.n, h.idx.p, h.flag.p);
        if (!m.hist_flag_scan(0, n, err)) return false;
        hist_scatter_kernel<<<g, 256, 0, m.stream>>>(h.items.p, h.splits.p, h.flag.p, h.scan.p, h.idx.p, h.idx_o.p);
        hist_copy_kernel<<<g, 256, 0, m.stream>>>(h.items.p, h.idx_o.p, h.idx.p);
        FR_HIP(hipGetLastError());
    }
    if (next_slots == 0) return true;
    // the next level's histograms: the smaller child of every pair from its stretch, the larger by subtraction
    if (!hist_level_alloc(h.cnt_o, h.sum_o, h.wsum_o, (size_t)next_slots * fk, newton, err)) return false;
    unsigned long long* const wsum_o = newton ? h.wsum_o.p : nullptr;
    if (!m.hist_zero(h.cnt_o.p, h.sum_o.p, wsum_o, 0, (size_t)next_slots * fk, err)) return false;
    std::vector<HistItemDev> stretches(builds.size());
    for (size_t i = 0; i < builds.size(); i++) {
        if (builds[i].slot >= next_slots || builds[i].end > n || builds[i].begin > builds[i].end)
            return hist_fail(err, "internal error: a child outside the next level");
        stretches[i] = {builds[i].slot, builds[i].begin, builds[i].end};
    }
    if (!m.hist_items(stretches, h.items_bh, h.items_b, err)) return false;
    if (!h.items_bh.empty()) m.hist_build(h.cnt_o.p, h.sum_o.p, wsum_o);
    if (!subs.empty()) {
        h.subs_h.resize(subs.size());
        for (size_t i = 0; i < subs.size(); i++) {
            if ((size_t)(subs[i].parent + 1) * fk > h.cnt.cap || (newton && (size_t)(subs[i].parent + 1) * fk > h.wsum.cap) || subs[i].small >= next_slots || subs[i].large >= next_slots)
                return hist_fail(err, "internal error: a subtraction outside the histograms");
            h.subs_h[i] = {subs[i].parent, subs[i].small, subs[i].large};
        }
        if (!h.subs.ensure(subs.size(), err)) return false;
        FR_HIP(hipMemcpyAsync(h.subs.p, h.subs_h.data(), subs.size() * sizeof(HistSubDev), hipMemcpyHostToDevice, m.stream));
        if (newton) {
            ProfScope ps("hist_sub_newton_kernel", m.stream);
            hist_sub_newton_kernel<<<dim3((unsigned)subs.size(), (unsigned)((fk + 255) / 256)), 256, 0, m.stream>>>(
                h.subs.p, (uint32_t)fk, h.cnt.p, h.sum.p, h.wsum.p, h.cnt_o.p, h.sum_o.p, h.wsum_o.p);
        } else {
            ProfScope ps("hist_sub_kernel", m.stream);
            hist_sub_kernel<<<dim3((unsigned)subs.size(), (unsigned)((fk + 255) / 256)), 256, 0, m.stream>>>(h.subs.p, (uint32_t)fk, h.cnt.p, h.sum.p,
                                                                                                           h.cnt_o.p, h.sum_o.p);
        }
    }
    FR_HIP(hipGetLastError());
    std::swap(h.cnt.p, h.cnt_o.p), std::swap(h.cnt.cap, h.cnt_o.cap);
    std::swap(h.sum.p, h.sum_o.p), std::swap(h.sum.cap, h.sum_o.cap);
    if (newton) std::swap(h.wsum.p, h.wsum_o.p), std::swap(h.wsum.cap, h.wsum_o.cap);
    return true;
}

bool DeviceDataset::hist_leaf_sums(const std::vector<HistNode>& leaves, std::vector<long long>* qw, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    const size_t L = leaves.size();
    qw->assign(L * 2, 0);
    if (L == 0) return true;
    std::vector<HistItemDev> stretches(L);
    for (size_t i = 0; i < L; i++) {
        if (leaves[i].end > h.tree_n() || leaves[i].begin > leaves[i].end) return hist_fail(err, "internal error: a leaf outside the index list");
        stretches[i] = {(uint32_t)i, leaves[i].begin, leaves[i].end};
    }
    FR_HIP(hipStreamSynchronize(m.stream));  // (hist.items is about to be rewritten)
    if (!h.leaf.ensure(L * 2, err) || !m.hist_items(stretches, h.items_h, h.items, err)) return false;
    FR_HIP(hipMemsetAsync(h.leaf.p, 0, L * 2 * sizeof(unsigned long long), m.stream));
    if (!h.items_h.empty()) {
        ProfScope ps("hist_leafsum_kernel", m.stream);
        hist_leafsum_kernel<<<(unsigned)h.items_h.size(), 256, 0, m.stream>>>(h.items.p, h.idx.p, h.Q.p, h.W.p, h.leaf.p);
    }
    FR_HIP(hipGetLastError());
    FR_HIP(hipMemcpyAsync(qw->data(), h.leaf.p, L * 2 * sizeof(long long), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    return true;
}

void DeviceDataset::hist_end() {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    auto& h = m.hist;
    (void)hipStreamSynchronize(m.stream);
    h.cnt.release(), h.cnt_o.release(), h.sum.release(), h.sum_o.release(), h.wsum.release(), h.wsum_o.release(), h.best.release(), h.best_n.release(), h.best_sym.release(), h.lam_in.release(), h.wt_in.release();
    h.pcnt.release(), h.psum.release(), h.pwsum.release(), h.rec.release(), h.pick.release(), h.bounds.release(), h.regn.release();
    h.pool_slots = 0;
}

// --- leaf-wise growth (kernels_hist.inc, "Leaf-wise growth") ---

// scan (after deriving where asked) and pick of `count` children, their records to out[0..count); waits for the stream
bool DeviceDataset::Impl::hist_leaf_scan(const HistLeafKids& kids, uint32_t count, const DeviceDataset::HistSearch& how,
                                         DeviceDataset::HistCand* out, std::string* err, const HistLeafBoundsDev* bounds, const HistLeafRegDev* reg) {
    static_assert(sizeof(DeviceDataset::HistCand) == sizeof(HistPickDev), "host and device records differ");
    auto& h = hist;
    if (!h.rec.ensure((size_t)2 * h.Ft, err) || !h.pick.ensure(2, err)) return false;
    const uint32_t* fsel = h.f_sampled ? h.fsel.p : nullptr;
    if (how.reg()) {
        if (!how.newton || reg == nullptr || h.mono_F == 0 || h.mono_F != h.F)
            return hist_fail(err, "internal error: no monotone signs set for these bins");
        ProfScope ps("hist_leaf_scan_reg_kernel", stream);
        hist_leaf_scan_reg_kernel<<<dim3(h.Ft, count), 64, 0, stream>>>(kids, *reg, h.Ft, h.k, h.nedges.p, h.mono.p, fsel, h.pcnt.p, h.psum.p, h.pwsum.p,
                                                                        how.min_leaf, how.s_l, how.s_w, hist_reg_numbers(how), h.rec.p);
    } else if (how.monotone) {
        if (!how.newton || bounds == nullptr || h.mono_F == 0 || h.mono_F != h.F)
            return hist_fail(err, "internal error: no monotone signs set for these bins");
        ProfScope ps("hist_leaf_scan_monotone_kernel", stream);
        hist_leaf_scan_monotone_kernel<<<dim3(h.Ft, count), 64, 0, stream>>>(kids, *bounds, h.Ft, h.k, h.nedges.p, h.mono.p, fsel, h.pcnt.p, h.psum.p,
                                                                             h.pwsum.p, how.min_leaf, how.s_l, how.s_w, how.lambda_l2,
                                                                             how.min_sum_hessian, h.rec.p);
    } else {
        ProfScope ps(how.newton ? "hist_leaf_scan_kernel<newton>" : "hist_leaf_scan_kernel", stream);
        const dim3 grid(h.Ft, count);
        if (how.newton)
            hist_leaf_scan_kernel<true><<<grid, 64, 0, stream>>>(kids, h.Ft, h.k, h.nedges.p, fsel, h.pcnt.p, h.psum.p, h.pwsum.p, how.min_leaf,
                                                                 how.s_l, how.s_w, how.lambda_l2, how.min_sum_hessian, h.rec.p);
        else
            hist_leaf_scan_kernel<false><<<grid, 64, 0, stream>>>(kids, h.Ft, h.k, h.nedges.p, fsel, h.pcnt.p, h.psum.p, nullptr, how.min_leaf, 0, 0,
                                                                  0.0, 0.0, h.rec.p);
    }
    {
        ProfScope ps("hist_pick_kernel", stream);
        hist_pick_kernel<<<count, 64, 0, stream>>>(h.rec.p, h.Ft, h.pick.p);
    }
    FR_HIP(hipGetLastError());
    FR_HIP(hipMemcpyAsync(out, h.pick.p, count * sizeof(HistPickDev), hipMemcpyDeviceToHost, stream));
    FR_HIP(hipStreamSynchronize(stream));
    return true;
}

bool DeviceDataset::hist_leaf_begin(uint32_t slots, const HistSearch& how, HistCand* root, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    if (h.k == 0) return hist_fail(err, "no bins built");
    if (slots == 0) return hist_fail(err, "internal error: an empty histogram pool");
    const size_t cells = (size_t)slots * h.Ft * h.k;
    if (!h.idx.ensure(h.n, err) || !h.idx_o.ensure(h.n, err) || !h.flag.ensure(h.n, err) || !h.scan.ensure(h.n, err)) return false;
    {
        std::string e2;
        if (!h.pcnt.ensure(cells, &e2) || !h.psum.ensure(cells, &e2) || (how.newton && !h.pwsum.ensure(cells, &e2))) {
            (void)hipGetLastError();
            h.pool_slots = 0;
            return hist_fail(err, "no device memory for the leaf-wise histogram pool (" + std::to_string((cells * (how.newton ? 20 : 12)) >> 20) +
                                      " MB: max_leaves x features x bins x " + (how.newton ? "20" : "12") + " bytes); lower max_leaves or split_candidates");
        }
    }
    h.pool_slots = slots;
    if (!m.hist_root_build(h.pcnt.p, h.psum.p, how.newton ? h.pwsum.p : nullptr, err)) return false;
    HistLeafKids kids{};
    kids.slot[0] = 0, kids.n[0] = h.tree_n();
    HistLeafBoundsDev whole{};  // (the root's interval: the whole line)
    whole.lo[0] = whole.lo[1] = -std::numeric_limits<double>::infinity();
    whole.hi[0] = whole.hi[1] = std::numeric_limits<double>::infinity();
    HistLeafRegDev rootless{};  // (and no parent)
    rootless.lo[0] = rootless.lo[1] = whole.lo[0], rootless.hi[0] = rootless.hi[1] = whole.hi[0];
    return m.hist_leaf_scan(kids, 1, how, root, err, &whole, &rootless);
}

bool DeviceDataset::hist_leaf_step(const HistLeafStep& step, const HistSearch& how, HistCand pick[2], std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& h = m.hist;
    const HistSplit& s = step.split;
    const size_t fk = (size_t)h.Ft * h.k;
    const bool build = step.small_slot != HIST_NO_SLOT;
    if (s.begin >= s.end || s.end > h.tree_n() || s.nl == 0 || s.nl >= s.end - s.begin || s.fslot >= h.F || s.edge >= h.k)
        return hist_fail(err, "internal error: a split outside the index list");
    if (h.pool_slots == 0 || step.parent_slot >= h.pool_slots || (build && (step.small_slot >= h.pool_slots || step.small_slot == step.parent_slot)) ||
        ((step.search_lhs || step.search_rhs) && !build))
        return hist_fail(err, "internal error: a step outside the histogram pool");
    const uint32_t n = s.end - s.begin, nr = n - s.nl;
    {
        ProfScope ps("hist_leaf_partition", m.stream);
        const dim3 g = grid1d(n, 256);
        hist_leaf_flag_kernel<<<g, 256, 0, m.stream>>>(s.begin, s.end, h.xbin.p + (size_t)s.fslot * h.n, s.edge, h.idx.p, h.flag.p);
        if (!m.hist_flag_scan(s.begin, n, err)) return false;
        hist_leaf_scatter_kernel<<<g, 256, 0, m.stream>>>(s.begin, s.end, s.nl, h.flag.p, h.scan.p, h.idx.p, h.idx_o.p);
        FR_HIP(hipMemcpyAsync(h.idx.p + s.begin, h.idx_o.p + s.begin, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, m.stream));
        FR_HIP(hipGetLastError());
    }
    if (!build) return true;
    // the smaller child from its stretch (the lhs when the two are equal)
    const bool left_small = s.nl <= nr;
    unsigned long long* const pwsum = how.newton ? h.pwsum.p : nullptr;
    if (!m.hist_zero(h.pcnt.p, h.psum.p, pwsum, (size_t)step.small_slot * fk, fk, err)) return false;
    const uint32_t mid = s.begin + s.nl;
    if (!m.hist_items({left_small ? HistItemDev{step.small_slot, s.begin, mid} : HistItemDev{step.small_slot, mid, s.end}}, h.items_bh, h.items_b, err))
        return false;
    m.hist_build(h.pcnt.p, h.psum.p, pwsum);
    FR_HIP(hipGetLastError());
    // the children to scan, the lhs first; the larger one is derived in place in its parent's slot
    HistLeafKids kids{};
    HistLeafBoundsDev bounds{};
    HistLeafRegDev reg{};
    uint32_t count = 0;
    int where[2] = {-1, -1};
    for (int side = 0; side < 2; side++) {
        if (!(side == 0 ? step.search_lhs : step.search_rhs)) continue;
        const bool small = (side == 0) == left_small;
        kids.slot[count] = small ? step.small_slot : step.parent_slot;
        kids.n[count] = side == 0 ? s.nl : nr;
        kids.derive[count] = small ? 0u : 1u;
        kids.other[count] = step.small_slot;
        bounds.lo[count] = reg.lo[count] = step.bounds[side].lo, bounds.hi[count] = reg.hi[count] = step.bounds[side].hi;
        reg.parent[count] = step.parent_out, reg.has_parent[count] = 1u;
        where[side] = (int)count++;
    }
    if (count == 0) return true;
    HistCand got[2];
    if (!m.hist_leaf_scan(kids, count, how, got, err, &bounds, &reg)) return false;
    for (int side = 0; side < 2; side++)
        if (where[side] >= 0) pick[side] = got[where[side]];
    return true;
}
