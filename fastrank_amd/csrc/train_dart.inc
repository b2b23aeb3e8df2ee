// Part of device.hip (single translation unit; see that file's header).  LambdaMART's DART boosting: the launchers of kernels_dart.inc.
// ----------------------------------------------------------------------------------------------
// LambdaMART's DART boosting (kernels_dart.inc)
// ----------------------------------------------------------------------------------------------
static bool dart_fail(std::string* err, const std::string& what) {
    if (err) *err = "LambdaMART DART: " + what;
    return false;
}

bool DeviceDataset::dart_begin(size_t rows, uint64_t* cache_bytes, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    Impl::DartState& d = m.dart;
    d.rows = d.filled = 0;
    d.stride = m.pos_threads();
    d.vals_h.clear();
    d.voff_h.assign(1, 0u);
    if (rows == 0 || d.stride == 0 || d.stride % 64 != 0) return dart_fail(err, "no trees or no documents to cache leaves for");
    if (d.stride > 0xFFFFFFFFull - (size_t)DART_MAX_GRID * DART_BLOCK * DART_DOCS) return dart_fail(err, "too many documents for the kernel's 32-bit document index");
    const size_t need = rows * d.stride;  // u16 entries
    if (need > d.leaf.cap) {
        // the one large allocation of a training: checked against what is free (with room for the growers' scratch) first
        const size_t free_b = device_free_bytes(), margin = (size_t)256 << 20;
        d.leaf.release();
        if (free_b != 0 && need * sizeof(uint16_t) + margin > free_b)
            return dart_fail(err, "the leaf cache of " + std::to_string(rows) + " trees x " + std::to_string(d.stride) + " documents needs " +
                                      std::to_string(need * sizeof(uint16_t)) + " bytes, " + std::to_string(free_b) + " are free on the device");
        if (!d.leaf.ensure(need, err)) return false;
    }
    if (!d.voff.ensure(rows + 1, err) || !d.w.ensure(rows, err) || !d.trees.ensure(rows, err) || !d.bad.ensure(1, err)) return false;
    if (!m.scores.ensure(m.np, err) || !m.acc.ensure(m.np, err)) return false;
    FR_HIP(hipMemsetAsync(d.voff.p, 0, sizeof(uint32_t), m.stream));
    FR_HIP(hipMemsetAsync(d.bad.p, 0, sizeof(int), m.stream));
    d.rows = rows;
    if (cache_bytes) *cache_bytes = (uint64_t)(need * sizeof(uint16_t));
    return true;
}

bool DeviceDataset::dart_fill(size_t row, const double* leaf_values, size_t n_leaves, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    Impl::DartState& d = m.dart;
    if (row != d.filled || row >= d.rows) return dart_fail(err, "the leaf cache is filled one tree after the other (row " + std::to_string(row) + ")");
    if (n_leaves == 0 || n_leaves > DART_MAX_LEAVES)
        return dart_fail(err, "a tree of " + std::to_string(n_leaves) + " leaves does not fit the leaf cache's 16-bit entries (at most 65536)");
    if (m.scores_slots < 1) return dart_fail(err, "no leaf numbers in score slot 0");
    // the leaf values join the table (a table that has to grow is uploaded again as a whole)
    FR_HIP(hipStreamSynchronize(m.stream));  // (earlier copies out of vals_h are done before it may move)
    const size_t at = d.vals_h.size();
    d.vals_h.insert(d.vals_h.end(), leaf_values, leaf_values + n_leaves);
    d.voff_h.push_back((uint32_t)d.vals_h.size());
    if (d.vals_h.size() > d.vals.cap) {
        if (!d.vals.ensure(std::max<size_t>(2 * d.vals_h.size(), 4096), err)) return false;
        FR_HIP(hipMemcpyAsync(d.vals.p, d.vals_h.data(), d.vals_h.size() * sizeof(double), hipMemcpyHostToDevice, m.stream));
    } else {
        FR_HIP(hipMemcpyAsync(d.vals.p + at, d.vals_h.data() + at, n_leaves * sizeof(double), hipMemcpyHostToDevice, m.stream));
    }
    FR_HIP(hipMemcpyAsync(d.voff.p + row + 1, d.voff_h.data() + row + 1, sizeof(uint32_t), hipMemcpyHostToDevice, m.stream));
    {
        ProfScope ps("dart_fill_kernel", m.stream);
        dart_fill_kernel<<<grid1d(d.stride, 256), 256, 0, m.stream>>>(m.scores.p, m.posmap(), (uint32_t)d.stride, (uint32_t)n_leaves, m.perm.p,
                                                                     d.leaf.p + row * d.stride, d.bad.p);
    }
    FR_HIP(hipGetLastError());
    int bad = 0;
    FR_HIP(hipMemcpyAsync(&bad, d.bad.p, sizeof(int), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    if (bad) {
        FR_HIP(hipMemsetAsync(d.bad.p, 0, sizeof(int), m.stream));
        return dart_fail(err, "a document was routed to no leaf of the tree");
    }
    d.filled = row + 1;
    return true;
}

bool DeviceDataset::dart_rescore(const double* weights, size_t n_weights, const uint32_t* trees, size_t n_trees, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    Impl::DartState& d = m.dart;
    if (d.rows == 0) return dart_fail(err, "no leaf cache");
    if (n_weights > d.filled || n_trees > d.rows) return dart_fail(err, "more weights or trees than the leaf cache has rows");
    for (size_t k = 0; k < n_trees; k++)
        if (trees[k] >= n_weights || (k > 0 && trees[k] <= trees[k - 1]))
            return dart_fail(err, "the tree list must be ascending and name trees that have a weight and a cache row");
    FR_HIP(hipStreamSynchronize(m.stream));  // (the staging copies of the last call are done)
    d.w_h.assign(weights, weights + n_weights);
    d.trees_h.assign(trees, trees + n_trees);
    if (n_weights) FR_HIP(hipMemcpyAsync(d.w.p, d.w_h.data(), n_weights * sizeof(double), hipMemcpyHostToDevice, m.stream));
    if (n_trees) FR_HIP(hipMemcpyAsync(d.trees.p, d.trees_h.data(), n_trees * sizeof(uint32_t), hipMemcpyHostToDevice, m.stream));
    const uint32_t n_vals = (uint32_t)d.vals_h.size();
    const bool in_lds = n_vals <= DART_LDS_VALUES;  // (else the lanes gather the leaf values from global memory)
    const dim3 grid(std::min<unsigned>(grid1d(d.stride, DART_BLOCK * DART_DOCS).x, DART_MAX_GRID));
    {
        ProfScope ps("dart_rescore_kernel", m.stream);
        if (in_lds)
            dart_rescore_kernel<true><<<grid, DART_BLOCK, (size_t)n_vals * sizeof(double), m.stream>>>(
                d.leaf.p, (uint32_t)d.stride, d.vals.p, d.voff.p, n_vals, d.w.p, d.trees.p, (uint32_t)n_trees, m.posmap(), m.scores.p, m.acc.p);
        else
            dart_rescore_kernel<false><<<grid, DART_BLOCK, 0, m.stream>>>(
                d.leaf.p, (uint32_t)d.stride, d.vals.p, d.voff.p, n_vals, d.w.p, d.trees.p, (uint32_t)n_trees, m.posmap(), m.scores.p, m.acc.p);
    }
    FR_HIP(hipGetLastError());
    m.scores_slots = 1;
    return true;
}

bool DeviceDataset::dart_download_row(size_t row, uint16_t* out_by_instance, size_t out_len, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    Impl::DartState& d = m.dart;
    if (row >= d.filled) return dart_fail(err, "no such row in the leaf cache");
    std::vector<uint16_t> tmp(d.stride);
    FR_HIP(hipMemcpyAsync(tmp.data(), d.leaf.p + row * d.stride, d.stride * sizeof(uint16_t), hipMemcpyDeviceToHost, m.stream));
    std::vector<uint32_t> tiles(m.nvtiles);
    if (m.nvtiles) FR_HIP(hipMemcpyAsync(tiles.data(), m.vtiles.p, m.nvtiles * sizeof(uint32_t), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    for (size_t i = 0; i < d.stride; i++) {
        const size_t p = m.nvtiles ? (size_t)tiles[i >> 6] * 64 + (i & 63) : i;
        const size_t id = m.perm_host[p];
        if (id != IDX_INVALID && id < out_len) out_by_instance[id] = tmp[i];
    }
    return true;
}

void DeviceDataset::dart_end() {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    (void)hipSetDevice(m.device);
    if (m.stream) (void)hipStreamSynchronize(m.stream);
    Impl::DartState& d = m.dart;
    d.leaf.release(), d.vals.release(), d.w.release(), d.voff.release(), d.trees.release(), d.bad.release();
    d.rows = d.filled = d.stride = 0;
    d.vals_h.clear(), d.voff_h.clear(), d.w_h.clear(), d.trees_h.clear();
}

