// Part of device.hip (single translation unit; see that file's header).  Random-forest training: the launchers of kernels_rf.inc.
// ----------------------------------------------------------------------------------------------
// random-forest training (kernels_rf.inc)
// ----------------------------------------------------------------------------------------------
void DeviceDataset::Impl::rf_args(RFArgs& a) {
    a.xb = xb.p;
    a.gain = rf.targets != nullptr ? rf.targets : gain.p;
    a.dq = (uint32_t)dq;
    a.roff = rf.roff.p;
    a.pos = rf.pos.p;
    a.gain_r = rf.gain_r.p;
    a.node_of = rf.node_of.p;
    a.side_r = rf.side_r.p;
    a.feats = rf.feats.p;
    a.T = rf.T;
    a.nf = rf.nf;
    a.total = rf.total;
    a.slot_of_key = rf.slot_of_key.p;
    a.A = rf.A;
    a.act_tree = rf.act_tree.p;
    a.act_n = rf.act_n.p;
    a.act_off = rf.act_off.p;
    a.keys = rf.keys_a.p;
    a.vals = rf.vals_a.p;
    a.skeys = rf.keys_b.p;
    a.svals = rf.vals_b.p;
    a.sg = rf.sg.p;
    a.sv = rf.sv.p;
    a.sg_o = rf.sg_o.p;
    a.sv_o = rf.sv_o.p;
    a.pres = rf.pw ? rf.pres.p : nullptr;
    a.pw = rf.pw;
    const char* int_env = frdev::path_env("FR_RF_INT_SUMS");
    const bool int_off = int_env != nullptr && int_env[0] == '0';
    a.labels_int = (labels_small_int && !int_off && a.gain == gain.p) ? 1u : 0u;
}

// which features every instance holds, by instance id ([n_instances][words]; nullptr / 0 words: all of them): random-forest
// training places its thresholds on the range of the HELD values (src/normalizers.rs:24-29)
bool DeviceDataset::rf_set_presence(const uint32_t* bits_by_instance, size_t words, size_t n_instances, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& rf = m.rf;
    rf.pw = 0;
    if (bits_by_instance == nullptr || words == 0) return true;
    std::vector<uint32_t> by_pos(m.np * words, 0xFFFFFFFFu);  // (padding positions are never sampled)
    for (size_t p = 0; p < m.np; p++) {
        const uint32_t id = m.perm_host[p];
        if (id != IDX_INVALID && id < n_instances) std::memcpy(&by_pos[p * words], bits_by_instance + (size_t)id * words, words * sizeof(uint32_t));
    }
    if (!upload(rf.pres, by_pos, err)) return false;
    rf.pw = (uint32_t)words;
    return true;
}

bool DeviceDataset::rf_positions(const std::vector<uint32_t>& root_ids, uint32_t* positions, std::string* err) {
    Impl& m = *impl_;
    auto& rf = m.rf;
    {
        std::lock_guard<std::mutex> lk(rf.pos_mu);  // (its own lock: the device jobs of a batch hold m.mu for tens of milliseconds)
        if (rf.pos_of_id.empty()) {
            uint32_t maxid = 0;
            for (uint32_t id : m.perm_host)
                if (id != IDX_INVALID) maxid = std::max(maxid, id);
            rf.pos_of_id.assign((size_t)maxid + 1, IDX_INVALID);
            for (size_t p = 0; p < m.perm_host.size(); p++)
                if (m.perm_host[p] != IDX_INVALID) rf.pos_of_id[m.perm_host[p]] = (uint32_t)p;
        }
    }
    const std::vector<uint32_t>& tab = rf.pos_of_id;  // (read-only from here on)
    for (size_t g = 0; g < root_ids.size(); g++) {
        const uint32_t id = root_ids[g];
        if (id >= tab.size() || tab[id] == IDX_INVALID) {
            if (err) *err = "rf_begin: instance id outside the dataset";
            return false;
        }
        positions[g] = tab[id];
    }
    return true;
}

bool DeviceDataset::rf_begin(const std::vector<uint32_t>& root_off, const std::vector<uint32_t>& root_ids, uint32_t nf,
                             const std::vector<uint32_t>& feats, std::string* err, const uint32_t* positions, bool lambda_targets) {
    std::vector<uint32_t> pos_own;
    if (positions == nullptr) {
        pos_own.resize(root_ids.size());
        if (!rf_positions(root_ids, pos_own.data(), err)) return false;
        positions = pos_own.data();
    }
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& rf = m.rf;
    const size_t T = root_off.size() - 1, total = root_ids.size();
    if (T == 0 || nf == 0 || feats.size() != T * nf || root_off.back() != total || (uint64_t)total * nf >= (1ull << 31)) {
        if (err) *err = "rf_begin: bad batch shape";
        return false;
    }
    for (uint32_t f : feats)
        if (f >= m.d) {
            if (err) *err = "rf_begin: feature id outside the dataset";
            return false;
        }
    rf.T = (uint32_t)T;
    rf.nf = nf;
    rf.total = (uint32_t)total;
    rf.roff_h = root_off;
    const size_t items = total * (size_t)nf;
    if (!rf.roff.ensure(T + 1, err) || !rf.pos.ensure(std::max<size_t>(total, 1), err) || !rf.node_of.ensure(std::max<size_t>(total, 1), err) ||
        !rf.feats.ensure(T * nf, err) || !rf.keys_a.ensure(std::max<size_t>(items, 1), err) || !rf.keys_b.ensure(std::max<size_t>(items, 1), err) ||
        !rf.vals_a.ensure(std::max<size_t>(items, 1), err) || !rf.vals_b.ensure(std::max<size_t>(items, 1), err) ||
        !rf.sg.ensure(std::max<size_t>(items, 1), err) || !rf.sv.ensure(std::max<size_t>(items, 1), err) ||
        !rf.sg_o.ensure(std::max<size_t>(items, 1), err) || !rf.sv_o.ensure(std::max<size_t>(items, 1), err) ||
        !rf.gain_r.ensure(std::max<size_t>(total, 1), err) || !rf.side_r.ensure(std::max<size_t>(total, 1), err))
        return false;
    FR_HIP(hipMemcpyAsync(rf.roff.p, root_off.data(), (T + 1) * 4, hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemcpyAsync(rf.pos.p, positions, total * 4, hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemcpyAsync(rf.feats.p, feats.data(), T * nf * 4, hipMemcpyHostToDevice, m.stream));
    // (the instances' first node keys -- their tree's root, key t -- are written on the device: no second 4-byte-per-instance upload)
    if (lambda_targets && !m.lm.built) {
        if (err) *err = "rf_begin: no LambdaMART gradients computed";
        return false;
    }
    rf.targets = lambda_targets ? m.lm.target.p : m.gain.p;
    if (total != 0) rf_gainr_kernel<<<grid1d(total, 256), 256, 0, m.stream>>>(rf.targets, rf.pos.p, rf.roff.p, (uint32_t)T, rf.gain_r.p, rf.node_of.p, (uint32_t)total);
    FR_HIP(hipGetLastError());
    FR_HIP(hipStreamSynchronize(m.stream));
    rf.A = 0;
    rf.prev_items = 0;
    rf.prev_A = 0;
    rf.prev_act_n.clear();
    rf.splits_for_A = 0;
    return true;
}

bool DeviceDataset::rf_root_outputs(std::vector<double>* out, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& rf = m.rf;
    if (!rf.child.ensure(std::max<size_t>(rf.T, 2), err)) return false;
    RFArgs a;
    m.rf_args(a);
    {
        ProfScope ps("rf_rootsum_kernel", m.stream);
        rf_rootsum_kernel<<<dim3(rf.T), 64, 0, m.stream>>>(a, rf.child.p);
    }
    out->assign(rf.T, 0.0);
    FR_HIP(hipMemcpyAsync(out->data(), rf.child.p, rf.T * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    return true;
}

bool DeviceDataset::rf_level(const std::vector<RfActive>& active, const std::vector<uint32_t>& slot_of_key, uint32_t k, int method,
                             uint32_t min_leaf, std::vector<RfCand>* cands, std::vector<float>* label_minmax, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& rf = m.rf;
    const size_t A = active.size();
    cands->clear();
    label_minmax->clear();
    // (fewer than two split candidates: no thresholds, random_forest.rs:236 -- nothing is evaluated and a following
    // rf_split has nothing to move; the level's tables are only valid when they were uploaded for THIS set of nodes)
    rf.A = (A == 0 || k < 2) ? 0u : (uint32_t)A;
    if (rf.A == 0) return true;
    std::vector<uint32_t> act_tree(A), act_n(A);
    std::vector<uint64_t> act_off(A + 1, 0), act_first(A + 1, 0);
    for (size_t i = 0; i < A; i++) {
        act_tree[i] = active[i].tree;
        act_n[i] = active[i].n;
        act_off[i + 1] = act_off[i] + (uint64_t)active[i].n * rf.nf;
        act_first[i + 1] = act_first[i] + active[i].n;
    }
    rf.items = act_off[A];
    rf.node_items = act_first[A];
    const uint64_t ncand = (uint64_t)A * rf.nf * (k - 1);
    if ((uint64_t)A * rf.nf >= 0x7FFFFFFFull || ncand >= (1ull << 31)) {
        if (err) *err = "rf_level: too many segments";
        return false;
    }
    // the tables of the level before stay intact for rf_rekey_kernel (ensure() below may reallocate)
    std::swap(rf.act_tree.p, rf.act_tree_o.p), std::swap(rf.act_tree.cap, rf.act_tree_o.cap);
    std::swap(rf.act_n.p, rf.act_n_o.p), std::swap(rf.act_n.cap, rf.act_n_o.cap);
    std::swap(rf.act_off.p, rf.act_off_o.p), std::swap(rf.act_off.cap, rf.act_off_o.cap);
    if (!rf.slot_of_key.ensure(std::max<size_t>(slot_of_key.size(), 1), err) || !rf.act_tree.ensure(A, err) || !rf.act_n.ensure(A, err) ||
        !rf.act_off.ensure(A + 1, err) || !rf.act_first.ensure(A + 1, err) || !rf.cands.ensure(ncand, err) || !rf.label.ensure(A * 2, err))
        return false;
    FR_HIP(hipMemcpyAsync(rf.slot_of_key.p, slot_of_key.data(), slot_of_key.size() * 4, hipMemcpyHostToDevice, m.stream));
    RFArgs a;
    m.rf_args(a);
    const bool from_scratch = rf.prev_items == 0 || frdev::path_env("FR_RF_RESORT");
    // levels after the first: the children's segments by a stable partition of the parents' (kernels_rf.inc); FR_RF_PARTITION=0:
    // by rewriting the segment ids and a stable radix sort on them
    const char* part_env = frdev::path_env("FR_RF_PARTITION");  // (read per level: the tests compare both paths in one process)
    const bool partition_on = part_env == nullptr || part_env[0] != '0';
    const bool partition = !from_scratch && partition_on && rf.splits_for_A == rf.prev_A && rf.prev_act_n.size() == rf.prev_A;
    std::vector<uint64_t> tile_first;
    if (partition) {
        tile_first.assign((size_t)rf.prev_A + 1, 0);
        for (uint32_t i = 0; i < rf.prev_A; i++) tile_first[i + 1] = tile_first[i] + (uint64_t)rf.nf * ((rf.prev_act_n[i] + RF_PT - 1) / RF_PT);
        if (tile_first.back() >= 0x7FFFFFFFull || !rf.tile_first_o.ensure(tile_first.size(), err) || !rf.tile_cnt.ensure(std::max<size_t>(2 * tile_first.back(), 2), err) ||
            !rf.side.ensure(std::max<size_t>(rf.prev_items, 1), err))
            return false;
        FR_HIP(hipMemcpyAsync(rf.tile_first_o.p, tile_first.data(), tile_first.size() * 8, hipMemcpyHostToDevice, m.stream));
    } else if (!from_scratch) {  // (reads the PREVIOUS level's tables, which the copies below overwrite afterwards, in stream order)
        RFArgs ao = a;
        ao.act_tree = rf.act_tree_o.p;
        ao.act_n = rf.act_n_o.p;
        ao.act_off = rf.act_off_o.p;
        ProfScope ps("rf_rekey_kernel", m.stream);
        rf_rekey_kernel<<<grid1d(rf.prev_items, 256), 256, 0, m.stream>>>(ao, rf.prev_items, rf.prev_A, (uint32_t)A);
    }
    FR_HIP(hipMemcpyAsync(rf.act_tree.p, act_tree.data(), A * 4, hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemcpyAsync(rf.act_n.p, act_n.data(), A * 4, hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemcpyAsync(rf.act_off.p, act_off.data(), (A + 1) * 8, hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipMemcpyAsync(rf.act_first.p, act_first.data(), (A + 1) * 8, hipMemcpyHostToDevice, m.stream));
    const size_t all_items = (size_t)rf.total * rf.nf;
    if (from_scratch) {
        ProfScope ps("rf_key_kernel", m.stream);
        rf_key_kernel<<<grid1d(rf.total, 256), 256, 0, m.stream>>>(a);
    }
    if (partition) {
        // the previous level's sorted gains / values become the scatter's input, this level's are written beside them
        std::swap(rf.sg.p, rf.sg_o.p), std::swap(rf.sg.cap, rf.sg_o.cap);
        std::swap(rf.sv.p, rf.sv_o.p), std::swap(rf.sv.cap, rf.sv_o.cap);
        m.rf_args(a);
        RFPart pp;
        pp.o_tree = rf.act_tree_o.p;
        pp.o_n = rf.act_n_o.p;
        pp.o_off = rf.act_off_o.p;
        pp.o_tile_first = rf.tile_first_o.p;
        pp.o_A = rf.prev_A;
        pp.sp = rf.splits.p;
        pp.tile_cnt = rf.tile_cnt.p;
        pp.side = rf.side.p;
        const unsigned tiles = (unsigned)tile_first.back();
        {
            ProfScope ps("rf_part_count_kernel", m.stream);
            rf_part_count_kernel<<<dim3(tiles), 256, 0, m.stream>>>(a, pp);
        }
        {
            ProfScope ps("rf_part_scan_kernel", m.stream);
            rf_part_scan_kernel<<<dim3(rf.prev_A * rf.nf), 64, 0, m.stream>>>(a, pp);
        }
        {
            ProfScope ps("rf_part_scatter_kernel", m.stream);
            rf_part_scatter_kernel<<<dim3(tiles), 256, 0, m.stream>>>(a, pp);
        }
        FR_HIP(hipGetLastError());
        // the partition wrote keys_a / vals_a: they are the sorted arrays now
        std::swap(rf.keys_a.p, rf.keys_b.p), std::swap(rf.keys_a.cap, rf.keys_b.cap);
        std::swap(rf.vals_a.p, rf.vals_b.p), std::swap(rf.vals_a.cap, rf.vals_b.cap);
        m.rf_args(a);
    } else {
        // stable LSD radix sort of (segment << 32 | value bits), only the bits in use: all of them the first time,
        // the segment bits alone afterwards (the value order inside a node survives a stable sort by child)
        unsigned seg_bits = 1;
        while ((1ull << seg_bits) <= (uint64_t)A * rf.nf) seg_bits++;
        const size_t count = from_scratch ? all_items : (size_t)rf.prev_items;
        const unsigned begin_bit = from_scratch ? 0u : 32u;
        size_t temp_bytes = 0;
        FR_HIP(rocprim::radix_sort_pairs(nullptr, temp_bytes, rf.keys_a.p, rf.keys_b.p, rf.vals_a.p, rf.vals_b.p, count, begin_bit, 32u + seg_bits,
                                         m.stream));
        if (!rf.temp.ensure(std::max<size_t>(temp_bytes, 16), err)) return false;
        ProfScope ps("rf_radix_sort", m.stream);
        FR_HIP(rocprim::radix_sort_pairs((void*)rf.temp.p, temp_bytes, rf.keys_a.p, rf.keys_b.p, rf.vals_a.p, rf.vals_b.p, count, begin_bit,
                                         32u + seg_bits, m.stream));
    }
    rf.prev_act_n = act_n;
    rf.splits_for_A = 0;  // (set again by the rf_split that decides THIS level)
    rf.prev_items = rf.items;
    rf.prev_A = (uint32_t)A;
    if (!partition) {  // (the partition's scatter writes the sorted gains and values itself)
        ProfScope ps("rf_gather_kernel", m.stream);
        rf_gather_kernel<<<grid1d(rf.items, 256), 256, 0, m.stream>>>(a, rf.items);
    }
    {
        ProfScope ps("rf_label_kernel", m.stream);
        rf_label_kernel<<<dim3((unsigned)A), RF_LABEL_THREADS, 0, m.stream>>>(a, rf.label.p);
    }
    {
        ProfScope ps("rf_eval_kernel", m.stream);
        rf_eval_kernel<<<dim3((unsigned)(A * rf.nf)), 64, 0, m.stream>>>(a, k, method, min_leaf, rf.cands.p);
    }
    FR_HIP(hipGetLastError());
    static_assert(sizeof(RfCand) == sizeof(RfCandDev), "host / device candidate records differ");
    cands->resize(ncand);
    label_minmax->resize(A * 2);
    FR_HIP(hipMemcpyAsync(cands->data(), rf.cands.p, ncand * sizeof(RfCandDev), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(label_minmax->data(), rf.label.p, A * 2 * sizeof(float), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    return true;
}

bool DeviceDataset::rf_split(const std::vector<RfSplit>& splits, std::vector<double>* child_out, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& rf = m.rf;
    const size_t A = rf.A;
    if (child_out) child_out->assign(splits.size() * 2, 0.0);  // (nullptr: the caller has the children's sums from the candidates, method 0)
    if (A == 0 || rf.node_items == 0) return true;
    if (splits.size() != A) {
        if (err) *err = "rf_split: one decision per active node expected";
        return false;
    }
    static_assert(sizeof(RfSplit) == sizeof(RfSplitDev), "host / device split records differ");
    if (!rf.splits.ensure(A, err) || !rf.child.ensure(std::max<size_t>(A * 2, rf.T), err)) return false;
    FR_HIP(hipMemcpyAsync(rf.splits.p, splits.data(), A * sizeof(RfSplitDev), hipMemcpyHostToDevice, m.stream));
    rf.splits_for_A = (uint32_t)A;
    RFArgs a;
    m.rf_args(a);
    {
        ProfScope ps("rf_assign_kernel", m.stream);
        rf_assign_kernel<<<grid1d(rf.node_items, 256), 256, 0, m.stream>>>(a, rf.splits.p, rf.node_items, rf.act_first.p);
    }
    if (child_out) {
        ProfScope ps("rf_childsum_kernel", m.stream);
        rf_childsum_kernel<<<dim3((unsigned)A), 64, 0, m.stream>>>(a, rf.splits.p, rf.child.p);
    }
    FR_HIP(hipGetLastError());
    if (child_out) FR_HIP(hipMemcpyAsync(child_out->data(), rf.child.p, A * 2 * sizeof(double), hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));  // (also without child sums: `splits` is the caller's pageable memory)
    return true;
}

bool DeviceDataset::rf_debug_sorted(std::vector<uint32_t>* svals, std::vector<float>* sv, std::vector<float>* sg, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    auto& rf = m.rf;
    const size_t items = rf.A == 0 ? 0 : (size_t)rf.items;
    svals->assign(items, 0u), sv->assign(items, 0.0f), sg->assign(items, 0.0f);
    if (items == 0) return true;
    RFArgs a;
    m.rf_args(a);
    FR_HIP(hipMemcpyAsync(svals->data(), a.svals, items * 4, hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(sv->data(), a.sv, items * 4, hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipMemcpyAsync(sg->data(), a.sg, items * 4, hipMemcpyDeviceToHost, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    return true;
}

void DeviceDataset::rf_end() {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    auto& rf = m.rf;
    rf.keys_a.release(), rf.keys_b.release(), rf.vals_a.release(), rf.vals_b.release(), rf.sg.release(), rf.sv.release(), rf.sg_o.release(), rf.sv_o.release(), rf.temp.release(), rf.side.release(), rf.tile_cnt.release();
    rf.cands.release();
}

