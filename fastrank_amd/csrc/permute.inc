// Part of device.hip (single translation unit; see that file's header).  The launchers of kernels_permute.inc (DESIGN.md
// section 16): the source positions uploaded once per call, then per chunk of columns one scoring pass into score slots
// k * R + r, which metric_from_scores and reduce_means take as they take any B slots.  The trees' layout (TreeNodeDev,
// adjacent_children_layout) is forest_pack.hpp's, which device.hip includes ahead of every part.

struct PermuteState {
    DevBuf<uint32_t> src, feats, uses;
    DevBuf<double> member, w, tw;
    DevBuf<TreeNodeDev> nodes;
    DevBuf<int32_t> roots;
    uint32_t R = 0;
    size_t scores_cap0 = 0;  // what the score slots held before the call (permute_end gives back what it grew)
};

namespace {

constexpr size_t PERM_MAX_SLOTS = 32768;       // metric_sort_kernel takes the slots as a grid dimension
constexpr size_t PERM_LDS_ROWS = 150 * 1024;   // as tree_ensemble_kernel: rows in LDS up to here, else read from the tiles

template <int RC>
void permute_launch_linear(bool lds_rows, unsigned nblocks, size_t lds, hipStream_t st, const PermArgs& a, const double* w) {
    if (lds_rows) {
        (void)hipFuncSetAttribute((const void*)permute_linear_kernel<true, RC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        permute_linear_kernel<true, RC><<<nblocks, 64, lds, st>>>(a, w);
    } else {
        permute_linear_kernel<false, RC><<<nblocks, 64, 0, st>>>(a, w);
    }
}

}  // namespace

const uint32_t* DeviceDataset::position_instances(size_t* np) const {
    *np = impl_->np;
    return impl_->perm_host.data();
}

bool DeviceDataset::permute_begin(const uint32_t* src_pos, uint32_t R, PermuteStats* stats, std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (R == 0 || R > frpermute::MAX_REPEATS || m.np == 0) {
        if (err) *err = "permute_begin: a size outside the kernels' limits";
        return false;
    }
    for (size_t i = 0; i < (size_t)R * m.np; i++)
        if (src_pos[i] >= m.np) {
            if (err) *err = "permute_begin: a source position outside the dataset";
            return false;
        }
    auto stp = std::make_shared<PermuteState>();
    stp->R = R;
    stp->scores_cap0 = m.scores.cap;
    if (!stp->src.ensure((size_t)R * m.np, err)) return false;
    const auto t0 = std::chrono::steady_clock::now();
    FR_HIP(hipMemcpyAsync(stp->src.p, src_pos, (size_t)R * m.np * sizeof(uint32_t), hipMemcpyHostToDevice, m.stream));
    FR_HIP(hipStreamSynchronize(m.stream));
    if (stats) {
        stats->upload_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->gather_xcol = m.xcol.p != nullptr;
        stats->rows_in_lds = 64 * (m.dq * 4 + 1) * sizeof(float) <= PERM_LDS_ROWS;
    }
    m.permute = stp;
    return true;
}

size_t DeviceDataset::permute_chunk_features(size_t nfeat, uint32_t R, size_t max_slots, size_t sets) const {
    const Impl& m = *impl_;
    size_t slots = max_slots;
    if (slots == 0) {  // half of what is free, as exact_kernels sizes its rows: `sets` sets of score slots and a column of the result matrix per slot
        (void)hipSetDevice(m.device);
        const size_t budget = std::max<size_t>(size_t(1) << 30, (device_free_bytes() + m.scores.bytes()) / 2);
        slots = budget / (sets * m.np * sizeof(double) + m.nq * sizeof(double));
    }
    slots = std::min(slots, PERM_MAX_SLOTS);
    return std::max<size_t>(1, std::min(nfeat, slots / std::max<uint32_t>(1, R)));  // (a column's R repeats stay together: never under one column)
}

bool DeviceDataset::permute_score(const uint32_t* feats, size_t nf, const std::vector<PermuteMember>& members, bool ensemble, PermuteStats* stats,
                                  std::string* err) {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.bind(err)) return false;
    if (!m.permute || nf == 0 || (!ensemble && members.size() != 1)) {
        if (err) *err = "permute_score: no call in progress, or nothing to score";
        return false;
    }
    PermuteState& s = *m.permute;
    const size_t R = s.R, B = nf * R, dp = m.dq * 4;
    for (size_t k = 0; k < nf; k++)
        if (feats[k] >= m.d || (k > 0 && feats[k] <= feats[k - 1])) {
            if (err) *err = "permute_score: columns must ascend and lie inside the matrix";
            return false;
        }
    if (B > PERM_MAX_SLOTS) {
        if (err) *err = "permute_score: too many slots in one chunk";
        return false;
    }
    if (!m.scores.ensure(B * m.np, err) || !s.feats.ensure(nf, err) || (ensemble && !s.member.ensure(B * m.np, err))) return false;
    m.scores_slots = B;
    const auto t0 = std::chrono::steady_clock::now();
    FR_HIP(hipMemcpyAsync(s.feats.p, feats, nf * sizeof(uint32_t), hipMemcpyHostToDevice, m.stream));
    if (ensemble) FR_HIP(hipMemsetAsync(m.scores.p, 0, B * m.np * sizeof(double), m.stream));  // acc = +0.0 (ensemble_begin)
    PermArgs a;
    a.xb = m.xb.p, a.pm = m.posmap(), a.dq = (uint32_t)m.dq, a.d = (uint32_t)m.d, a.np = (uint32_t)m.np;
    a.xcol = m.xcol.p, a.src = s.src.p, a.feats = s.feats.p;
    a.nf = (uint32_t)nf, a.R = (uint32_t)R, a.r0 = 0;
    a.out = ensemble ? s.member.p : m.scores.p;
    const size_t lds = 64 * (dp + 1) * sizeof(float);
    const bool lds_rows = lds <= PERM_LDS_ROWS;
    const unsigned nblocks = (unsigned)(m.pos_threads() / 64);  // (np and a view's tile list are whole tiles)
    for (const PermuteMember& mb : members) {
        if (mb.kind == PermuteMember::LINEAR) {
            std::vector<double> wpad(dp, 0.0);
            std::memcpy(wpad.data(), mb.weights, m.d * sizeof(double));
            if (!s.w.ensure(dp, err)) return false;
            FR_HIP(hipMemcpyAsync(s.w.p, wpad.data(), dp * sizeof(double), hipMemcpyHostToDevice, m.stream));
            FR_HIP(hipStreamSynchronize(m.stream));  // wpad is a local
            ProfScope ps("permute_linear_kernel", m.stream);
            for (uint32_t r0 = 0; r0 < R; r0 += frpermute::ACC) {
                a.r0 = r0;
                switch (std::min<uint32_t>(frpermute::ACC, (uint32_t)R - r0)) {
                    case 1: permute_launch_linear<1>(lds_rows, nblocks, lds, m.stream, a, s.w.p); break;
                    case 2: permute_launch_linear<2>(lds_rows, nblocks, lds, m.stream, a, s.w.p); break;
                    case 3: permute_launch_linear<3>(lds_rows, nblocks, lds, m.stream, a, s.w.p); break;
                    case 4: permute_launch_linear<4>(lds_rows, nblocks, lds, m.stream, a, s.w.p); break;
                    case 5: permute_launch_linear<5>(lds_rows, nblocks, lds, m.stream, a, s.w.p); break;
                    case 6: permute_launch_linear<6>(lds_rows, nblocks, lds, m.stream, a, s.w.p); break;
                    case 7: permute_launch_linear<7>(lds_rows, nblocks, lds, m.stream, a, s.w.p); break;
                    default: permute_launch_linear<8>(lds_rows, nblocks, lds, m.stream, a, s.w.p); break;
                }
                if (stats) stats->launches_linear++;
            }
        } else if (mb.kind == PermuteMember::SINGLE) {
            ProfScope ps("permute_single_kernel", m.stream);
            permute_single_kernel<<<dim3((unsigned)((m.pos_threads() + 255) / 256), (unsigned)B), 256, 0, m.stream>>>(a, mb.fid, mb.dir);
            if (stats) stats->launches_single++;
        } else {
            const FlatTrees& t = *mb.trees;
            const size_t nt = t.root.size(), uw = (nf + 31) / 32;
            std::vector<TreeNodeDev> nodes;
            std::vector<int32_t> roots;
            adjacent_children_layout(t, nodes, roots);
            std::vector<double> tw = t.weight;
            tw.resize(nt, 1.0);
            std::vector<uint32_t> uses(std::max<size_t>(1, nt * uw), 0u);
            for (size_t k = 0; k < nt; k++) {
                const size_t end = k + 1 < nt ? (size_t)roots[k + 1] : nodes.size();
                for (size_t i = (size_t)roots[k]; i < end; i++) {
                    if (nodes[i].fid < 0) continue;
                    const uint32_t* at = std::lower_bound(feats, feats + nf, (uint32_t)nodes[i].fid);
                    if (at != feats + nf && *at == (uint32_t)nodes[i].fid) uses[k * uw + (size_t)(at - feats) / 32] |= 1u << ((at - feats) % 32);
                }
            }
            if (!s.nodes.ensure(std::max<size_t>(nodes.size(), 1), err) || !s.roots.ensure(std::max<size_t>(nt, 1), err) ||
                !s.tw.ensure(std::max<size_t>(nt, 1), err) || !s.uses.ensure(uses.size(), err))
                return false;
            FR_HIP(hipMemcpyAsync(s.nodes.p, nodes.data(), nodes.size() * sizeof(TreeNodeDev), hipMemcpyHostToDevice, m.stream));
            FR_HIP(hipMemcpyAsync(s.roots.p, roots.data(), nt * sizeof(int32_t), hipMemcpyHostToDevice, m.stream));
            FR_HIP(hipMemcpyAsync(s.tw.p, tw.data(), nt * sizeof(double), hipMemcpyHostToDevice, m.stream));
            FR_HIP(hipMemcpyAsync(s.uses.p, uses.data(), uses.size() * sizeof(uint32_t), hipMemcpyHostToDevice, m.stream));
            FR_HIP(hipStreamSynchronize(m.stream));  // the staging vectors are locals
            ProfScope ps("permute_trees_kernel", m.stream);
            if (lds_rows) FR_HIP(hipFuncSetAttribute((const void*)permute_trees_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            for (uint32_t r0 = 0; r0 < R; r0 += frpermute::ACC) {
                a.r0 = r0;
                const uint32_t rc = std::min<uint32_t>(frpermute::ACC, (uint32_t)R - r0);
                if (lds_rows)
                    permute_trees_kernel<true><<<nblocks, 64 * PERM_TREE_WAVES, lds, m.stream>>>(a, s.nodes.p, s.roots.p, s.tw.p, (uint32_t)nt, t.raw_single ? 1 : 0, s.uses.p, (uint32_t)uw, rc);
                else
                    permute_trees_kernel<false><<<nblocks, 64 * PERM_TREE_WAVES, 0, m.stream>>>(a, s.nodes.p, s.roots.p, s.tw.p, (uint32_t)nt, t.raw_single ? 1 : 0, s.uses.p, (uint32_t)uw, rc);
                if (stats) stats->launches_trees++;
            }
        }
        FR_HIP(hipGetLastError());
        if (ensemble) {
            ProfScope ps("permute_axpy_kernel", m.stream);
            permute_axpy_kernel<<<dim3((unsigned)((m.pos_threads() + 255) / 256), (unsigned)B), 256, 0, m.stream>>>(m.scores.p, s.member.p, m.posmap(), (uint32_t)m.np,
                                                                                                                 mb.ens_weight);
            FR_HIP(hipGetLastError());
            if (stats) stats->launches_axpy++;
        }
    }
    FR_HIP(hipStreamSynchronize(m.stream));
    if (stats) stats->score_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return true;
}

void DeviceDataset::permute_end() {
    Impl& m = *impl_;
    std::lock_guard<std::mutex> lk(m.mu);
    if (!m.permute) return;
    (void)hipSetDevice(m.device);
    (void)hipStreamSynchronize(m.stream);
    if (m.scores.cap > m.permute->scores_cap0) {  // the call's slots go back; whoever scores next allocates what it needs
        m.scores.release();
        m.scores_slots = 0;
    }
    m.permute.reset();
}
