// The host-side layout of a DeviceDataset: everything DeviceDataset::create / create_view compute
// before or between their uploads, as functions of plain vectors.  No HIP and no environment here: the callers read the
// switches (FR_RUN_DOCS, FR_NO_DUP_GROUPS) and hand the values in.  fr_debug_dataset_layout / native.host_layout serve
// every table below without a device; tests/test_device_form_host.py holds them to the numpy restatement.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace frdev {

constexpr uint32_t NO_DOCUMENT = 0xFFFFFFFFu;  // perm[p] of a position that holds no document (the kernels' IDX_INVALID)
constexpr int DCG_RANKS = 20;                  // ranks the per-gain-class DCG term table covers (the kernels' LS_KT)

struct HostCSR {
    size_t n = 0, d = 0, nq = 0;
    const float* x = nullptr;     // row-major base matrix, stride d
    std::vector<uint32_t> perm;   // CSR position -> row in x (original InstanceId)
    std::vector<uint32_t> qoff;   // [nq+1]
    std::vector<float> gain;      // [n] by CSR position
};

// Walk tiles of the resident NDCG@k verify kernel (kernels_order.inc).  Every run's positions are cut, greedily and in query
// order, into stretches of at most WALK_TILE positions such that a query of up to WALK_TILE documents is never cut; a longer
// one is cut every WALK_TILE documents from its start and what is left of it shares a tile with the queries behind it.
//   wt_start[i] = first position of tile i, ascending; one more entry = np (behind a run's last tile comes padding)
//   run_wt0[r]  = the tile run r starts in (tiles never span runs)
//   seg[p]      = first slot | (one past the last slot) << 8 of position p's (query, tile) segment, relative to the tile's
//                 start; 0 for positions that hold no document
//   wofs[p]     = p's offset inside its tile
constexpr uint32_t WALK_TILE = 128;
struct WalkTileLayout {
    std::vector<uint32_t> wt_start, run_wt0;
    std::vector<uint16_t> seg;
    std::vector<uint8_t> wofs;
};
inline WalkTileLayout build_walk_tiles(const std::vector<uint32_t>& run_pos, const std::vector<uint32_t>& run_q0, const std::vector<uint32_t>& run_q1,
                                       const std::vector<uint32_t>& qstart, const std::vector<uint32_t>& qlen, size_t np) {
    constexpr uint32_t WT = WALK_TILE;
    WalkTileLayout out;
    std::vector<uint32_t>& wts = out.wt_start;
    const size_t nruns = run_pos.size(), nq = qlen.size();
    out.run_wt0.assign(nruns, 0);
    for (size_t r = 0; r < nruns; r++) {
        out.run_wt0[r] = (uint32_t)wts.size();
        uint32_t start = run_pos[r], len = 0;
        auto close = [&]() {
            if (len == 0) return;
            wts.push_back(start);
            start += len;
            len = 0;
        };
        for (uint32_t q = run_q0[r]; q < run_q1[r]; q++) {
            uint32_t n = qlen[q];
            if (n > WT) {
                close();
                for (; n > WT; n -= WT) {
                    len = WT;
                    close();
                }
                len = n;
            } else {
                if (len + n > WT) close();
                len += n;
            }
        }
        close();
    }
    const size_t nwt = wts.size();
    wts.push_back((uint32_t)np);
    out.seg.assign(np, 0);
    out.wofs.assign(np, 0);
    size_t t = 0;
    for (size_t q = 0; q < nq; q++) {
        const size_t b = qstart[q], e = b + qlen[q];
        while (t + 1 < nwt && wts[t + 1] <= b) t++;
        for (size_t u = t; u < nwt && wts[u] < e; u++) {
            const size_t t0 = wts[u], t1 = std::min<size_t>((size_t)wts[u + 1], t0 + WT);
            const size_t lo = std::max(b, t0) - t0, hi = std::min(e, t1) - t0;
            for (size_t p = t0 + lo; p < t0 + hi; p++) {
                out.seg[p] = (uint16_t)(lo | (hi << 8));
                out.wofs[p] = (uint8_t)(p - t0);
            }
        }
    }
    return out;
}

// ---- runs: consecutive queries packed into whole 64-document tiles ----------------------------------------------------
// The query and run tables of a dataset, in a position space of np positions.  A view's (plan_view_runs) live in its
// parent's space: the tables behind `np` are filled for views alone.
struct RunPlan {
    std::vector<uint32_t> qstart, qlen, qtight, run_q0, run_q1, run_pos, run_docs, run_order;
    size_t np = 0, maxlen = 0;
    std::vector<uint32_t> run_lo;     // lane of a tile the run's first query starts at
    std::vector<uint32_t> vtiles;     // the 64-position tiles of the parent's position space that hold the view's documents (ascending)
    std::vector<uint32_t> run_wt0;    // the parent's walk tile each run starts in
    std::vector<uint32_t> wlist;      // the parent's walk tiles that hold the view's documents (ascending)
    std::vector<uint32_t> perm_host;  // [np] instance id, NO_DOCUMENT where the view has no document
};

// longest-first schedule so the biggest runs do not form the tail of a launch
inline std::vector<uint32_t> longest_first(const std::vector<uint32_t>& run_docs) {
    std::vector<uint32_t> order(run_docs.size());
    for (size_t r = 0; r < order.size(); r++) order[r] = (uint32_t)r;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return run_docs[x] > run_docs[y]; });
    return order;
}

// A dataset that owns its matrix: queries go into a run while it stays at or below `target` documents, packed tightly;
// every run starts on a multiple of 64.  false (with *err) when the position space does not fit 32 bits.
inline bool plan_runs(const std::vector<uint32_t>& qoff, size_t nq, size_t target, RunPlan* out, std::string* err) {
    RunPlan& r = *out;
    r.qstart.assign(nq, 0);
    r.qlen.assign(nq, 0);
    r.qtight.assign(nq + 1, 0);
    size_t pos = 0, cur_docs = 0;
    uint32_t cur_q0 = 0;
    auto close_run = [&](uint32_t q_end) {
        r.run_q0.push_back(cur_q0);
        r.run_q1.push_back(q_end);
        r.run_pos.push_back((uint32_t)(pos - cur_docs));
        r.run_docs.push_back((uint32_t)cur_docs);
        pos = (pos + 63) / 64 * 64;
        cur_docs = 0;
        cur_q0 = q_end;
    };
    for (size_t q = 0; q < nq; q++) {
        size_t len = qoff[q + 1] - qoff[q];
        r.maxlen = std::max(r.maxlen, len);
        if (cur_docs > 0 && cur_docs + len > target) close_run((uint32_t)q);
        r.qstart[q] = (uint32_t)pos;
        r.qlen[q] = (uint32_t)len;
        r.qtight[q] = qoff[q];
        pos += len;
        cur_docs += len;
    }
    if (cur_docs > 0) close_run((uint32_t)nq);
    r.qtight[nq] = qoff[nq];
    r.np = pos;
    if (r.np >= 0xFFFFFF00ull) {
        if (err) *err = "dataset too large for 32-bit document positions";
        return false;
    }
    r.run_order = longest_first(r.run_docs);
    return true;
}

// perm[p] = the instance id stored at position p
inline std::vector<uint32_t> position_map(const HostCSR& csr, const std::vector<uint32_t>& qstart, const std::vector<uint32_t>& qlen, size_t np) {
    std::vector<uint32_t> perm(np, NO_DOCUMENT);
    for (size_t q = 0; q < qlen.size(); q++)
        for (uint32_t k = 0; k < qlen[q]; k++) perm[(size_t)qstart[q] + k] = csr.perm[(size_t)csr.qoff[q] + k];
    return perm;
}

// A view: its queries inside the parent's position space (query q of the view is the parent's parent_query[q]); runs =
// maximal groups of queries that are consecutive there (and at most `target` documents), each starting wherever its first
// query starts: run_lo lanes into a tile.  parent_wt_start: the parent's walk tiles, np appended.
inline bool plan_view_runs(const std::vector<uint32_t>& parent_qstart, const std::vector<uint32_t>& parent_qlen,
                           const std::vector<uint32_t>& parent_perm_host, const std::vector<uint32_t>& parent_wt_start, const HostCSR& csr,
                           const std::vector<uint32_t>& parent_query, size_t target, RunPlan* out, std::string* err) {
    RunPlan& v = *out;
    const size_t nq = csr.nq;
    auto fail = [&](const char* msg) {
        if (err) *err = msg;
        return false;
    };
    v.np = parent_perm_host.size();  // the parent's position space
    v.qstart.assign(nq, 0);
    v.qlen.assign(nq, 0);
    v.qtight.assign(nq + 1, 0);
    v.perm_host.assign(v.np, NO_DOCUMENT);
    for (size_t q = 0; q < nq; q++) {
        const uint32_t pq = parent_query[q];
        const size_t len = csr.qoff[q + 1] - csr.qoff[q];
        if (pq >= parent_qlen.size() || parent_qlen[pq] != len) return fail("create_view: a query of the view differs from the parent's");
        v.qstart[q] = parent_qstart[pq];
        v.qlen[q] = (uint32_t)len;
        v.qtight[q] = csr.qoff[q];
        v.maxlen = std::max(v.maxlen, len);
        for (size_t k = 0; k < len; k++) {
            const uint32_t id = parent_perm_host[(size_t)v.qstart[q] + k];
            if (id != csr.perm[csr.qoff[q] + k]) return fail("create_view: document order inside a query differs from the parent's");
            v.perm_host[(size_t)v.qstart[q] + k] = id;
        }
    }
    v.qtight[nq] = csr.qoff[nq];
    // the tiles of the parent's position space this view touches: position-parallel kernels (exact scoring, resident
    // refreshes) visit only these
    {
        std::vector<char> touched((v.np + 63) / 64, 0);
        for (size_t q = 0; q < nq; q++)
            for (size_t t = v.qstart[q] >> 6; t <= ((size_t)v.qstart[q] + v.qlen[q] - 1) >> 6; t++) touched[t] = 1;
        for (size_t t = 0; t < touched.size(); t++)
            if (touched[t]) v.vtiles.push_back((uint32_t)t);
    }
    for (size_t q0 = 0; q0 < nq;) {
        size_t q1 = q0 + 1, docs = v.qlen[q0];
        while (q1 < nq && v.qstart[q1] == v.qstart[q1 - 1] + v.qlen[q1 - 1] && docs + v.qlen[q1] <= target) {
            docs += v.qlen[q1];
            q1++;
        }
        v.run_q0.push_back((uint32_t)q0);
        v.run_q1.push_back((uint32_t)q1);
        v.run_pos.push_back(v.qstart[q0] & ~63u);
        v.run_lo.push_back(v.qstart[q0] & 63u);
        v.run_docs.push_back((uint32_t)docs + (v.qstart[q0] & 63u));
        q0 = q1;
    }
    v.run_order = longest_first(v.run_docs);
    // the parent's walk tiles (kernels_order.inc) as this view meets them: the tile each run starts in, and the tiles that
    // hold the view's documents (the ones whose R ranks rslot_kernel keeps)
    const std::vector<uint32_t>& wts = parent_wt_start;
    const size_t nwt = wts.empty() ? 0 : wts.size() - 1;
    auto tile_of = [&](uint32_t p) { return (uint32_t)(std::upper_bound(wts.begin(), wts.begin() + nwt, p) - wts.begin() - 1); };
    v.run_wt0.assign(v.run_q0.size(), 0);
    for (size_t r = 0; r < v.run_q0.size(); r++) {
        const uint32_t first = v.qstart[v.run_q0[r]], last = v.qstart[v.run_q1[r] - 1] + v.qlen[v.run_q1[r] - 1] - 1u;
        v.run_wt0[r] = tile_of(first);
        for (uint32_t t = v.run_wt0[r], te = tile_of(last); t <= te; t++)
            if (v.wlist.empty() || v.wlist.back() < t) v.wlist.push_back(t);  // (runs ascend in position: so do their tiles)
    }
    return true;
}

// ---- size classes: queries sorted by class (stable: dataset order inside a class), then cut ------------------------------
struct SizeClass {
    uint32_t npad, offset, count;  // the class (whatever class_of returns), its stretch of the list
};
template <class ClassOf>
inline std::vector<SizeClass> bucket_queries(const std::vector<uint32_t>& qlen, ClassOf class_of, std::vector<uint32_t>* list) {
    const size_t nq = qlen.size();
    std::vector<uint32_t> cls(nq);
    for (size_t q = 0; q < nq; q++) cls[q] = (uint32_t)class_of(qlen[q]);
    list->resize(nq);
    for (size_t q = 0; q < nq; q++) (*list)[q] = (uint32_t)q;
    std::stable_sort(list->begin(), list->end(), [&](uint32_t x, uint32_t y) { return cls[x] < cls[y]; });
    std::vector<SizeClass> out;
    for (size_t k = 0; k < nq;) {
        const uint32_t c = cls[(*list)[k]];
        size_t e = k;
        while (e < nq && cls[(*list)[e]] == c) e++;
        out.push_back({c, (uint32_t)k, (uint32_t)(e - k)});
        k = e;
    }
    return out;
}
// the general (sort) evaluator's rule: LDS sized per class, not per dataset maximum
inline uint32_t pow2_from_64(uint32_t len) {
    uint32_t p2 = 64;
    while (p2 < len) p2 <<= 1;
    return p2;
}

// ---- padded per-position gains, gain classes and the term tables ---------------------------------------------------------
struct GainTables {
    std::vector<float> gain;            // [np]
    std::vector<double> gexp;           // [np] 2^gain - 1
    bool labels_small_int = true;       // every label is an integer of magnitude <= 2^21
    std::vector<uint32_t> gcls;         // [np] gain class, numbered by descending gain
    std::vector<float> cls_gain;        // [classes]
    uint64_t relmask = 0;               // bit c: gain class c has gain > 0
    std::vector<double> dcgtab;         // [classes][DCG_RANKS]
    std::vector<uint32_t> qnpos, qnneg; // [nq]
    std::vector<double> termtab;        // [ncls + 1][tablen], empty when there are too many classes or it would be too large
    size_t ncls = 0, tablen = 0;
};
// Three stages over one record, in this order (create() times each); gain_tables runs all three.
inline void position_gains(const HostCSR& csr, const std::vector<uint32_t>& qstart, const std::vector<uint32_t>& qlen, size_t np, GainTables* out) {
    GainTables& g = *out;
    const size_t nq = qlen.size();
    g.gain.assign(np, 0.0f);
    g.gexp.assign(np, 0.0);
    {
        // (2^g - 1) with the platform libm, exactly like 2.0_f64.powf(gain) - 1.0 (src/evaluators.rs:266-270); g is
        // the f32 gain widened to f64.  Labels repeat: one pow per distinct bit pattern.
        std::vector<std::pair<uint32_t, double>> memo;
        auto gexp_of = [&](float gv) {
            uint32_t bits;
            std::memcpy(&bits, &gv, sizeof(bits));
            for (const auto& e : memo)
                if (e.first == bits) return e.second;
            const double v = std::pow(2.0, (double)gv) - 1.0;
            if (memo.size() < 64) memo.emplace_back(bits, v);
            return v;
        };
        for (size_t q = 0; q < nq; q++) {
            for (uint32_t k = 0; k < qlen[q]; k++) {
                size_t p = (size_t)qstart[q] + k, t = (size_t)csr.qoff[q] + k;
                g.gain[p] = csr.gain[t];
                g.gexp[p] = gexp_of(csr.gain[t]);
                const float gl = csr.gain[t];
                if (!(std::fabs(gl) <= 2097152.0f) || gl != (float)(int32_t)gl) g.labels_small_int = false;
            }
        }
    }
}
// ---- gain classes and the per-class DCG term table: term(c, i) = (2^g_c - 1) / log2(i + 2), the
// exact expression of src/evaluators.rs:266-270 evaluated once per (class, rank) on the host
inline void gain_classes(const std::vector<uint32_t>& perm_host, GainTables* out) {
    GainTables& g = *out;
    const size_t np = perm_host.size();
    g.gcls.assign(np, 0);
    {
        // class ids in order of DESCENDING gain: among keys that agree above the class bits -- exact duplicates -- the
        // lower gain then has the larger key and sorts first, which is the reference's tie-break (gain asc, evaluators.rs:34-49)
        std::vector<float>& cls_gain = g.cls_gain;
        {
            std::vector<uint32_t> seen_bits;
            uint32_t last_bits = 0;
            bool have_last = false;
            for (size_t p = 0; p < np; p++) {
                if (perm_host[p] == NO_DOCUMENT) continue;
                const float gv = g.gain[p] == 0.0f ? 0.0f : g.gain[p];  // -0.0 and +0.0 are one class
                uint32_t bits;
                std::memcpy(&bits, &gv, sizeof(bits));
                if (have_last && bits == last_bits) continue;  // documents are stored gain-descending: long runs of one class
                last_bits = bits;
                have_last = true;
                if (std::find(seen_bits.begin(), seen_bits.end(), bits) == seen_bits.end()) {
                    if (seen_bits.size() > 4096) break;  // (far too many distinct gains for the class machinery: found below)
                    seen_bits.push_back(bits);
                    cls_gain.push_back(gv);
                }
            }
            std::sort(cls_gain.begin(), cls_gain.end(), [](float x, float y) { return x > y; });
        }
        std::map<uint32_t, uint32_t> cls_of_bits;
        for (size_t c = 0; c < cls_gain.size(); c++) {
            uint32_t bits;
            std::memcpy(&bits, &cls_gain[c], sizeof(bits));
            cls_of_bits.emplace(bits, (uint32_t)c);
        }
        uint32_t last_bits = 0, last_cls = 0;
        bool have_last = false;
        for (size_t p = 0; p < np; p++) {
            if (perm_host[p] == NO_DOCUMENT) continue;
            float gv = g.gain[p] == 0.0f ? 0.0f : g.gain[p];
            uint32_t bits;
            std::memcpy(&bits, &gv, sizeof(bits));
            if (!have_last || bits != last_bits) {
                auto it = cls_of_bits.find(bits);
                if (it == cls_of_bits.end()) {  // (only after the 4096 cut above: more classes than any fused path takes)
                    it = cls_of_bits.emplace(bits, (uint32_t)cls_gain.size()).first;
                    cls_gain.push_back(gv);
                }
                last_bits = bits;
                last_cls = it->second;
                have_last = true;
            }
            g.gcls[p] = last_cls;
        }
        if (cls_gain.empty()) cls_gain.push_back(0.0f);
        for (size_t c = 0; c < cls_gain.size() && c < 64; c++)
            if (cls_gain[c] > 0.0f) g.relmask |= uint64_t(1) << c;
        g.dcgtab.resize(cls_gain.size() * DCG_RANKS);
        for (size_t c = 0; c < cls_gain.size(); c++)
            for (int i = 0; i < DCG_RANKS; i++)
                g.dcgtab[c * DCG_RANKS + i] = (std::pow(2.0, (double)cls_gain[c]) - 1.0) / std::log2((double)i + 2.0);
    }
}
// per-query counts of positive / negative gains (documents are stored gain-descending, so these are a
// prefix / suffix of the query) and the full-depth term table for the rank-counting evaluator
inline void term_tables(const std::vector<uint32_t>& qstart, const std::vector<uint32_t>& qlen, size_t maxlen, GainTables* out) {
    GainTables& g = *out;
    const size_t nq = qlen.size();
    g.qnpos.assign(nq, 0);
    g.qnneg.assign(nq, 0);
    for (size_t q = 0; q < nq; q++)
        for (uint32_t k = 0; k < qlen[q]; k++) {
            float gv = g.gain[(size_t)qstart[q] + k];
            g.qnpos[q] += gv > 0.0f;
            g.qnneg[q] += gv < 0.0f;
        }
    g.ncls = g.dcgtab.size() / DCG_RANKS;
    // row length: the padded query length of the longest size class (kernels_fullverify.inc looks up every rank of
    // a padded query); one more row of zeros = the "padding class" its padding keys carry
    g.tablen = 16;
    while (g.tablen < maxlen) g.tablen <<= 1;
    if (g.ncls <= 255 && (g.ncls + 1) * g.tablen <= (size_t(64) << 20)) {
        g.termtab.assign((g.ncls + 1) * g.tablen, 0.0);
        for (size_t c = 0; c < g.ncls; c++) {
            const double ge = g.dcgtab[c * DCG_RANKS] * std::log2(2.0);  // = 2^g - 1 (term at rank 0, log2(2) = 1)
            for (size_t r = 0; r < g.tablen; r++) g.termtab[c * g.tablen + r] = ge / std::log2((double)r + 2.0);
        }
    }
}
inline GainTables gain_tables(const HostCSR& csr, const std::vector<uint32_t>& qstart, const std::vector<uint32_t>& qlen,
                              const std::vector<uint32_t>& perm_host, size_t maxlen) {
    GainTables g;
    position_gains(csr, qstart, qlen, perm_host.size(), &g);
    gain_classes(perm_host, &g);
    term_tables(qstart, qlen, maxlen, &g);
    return g;
}

// ---- duplicate groups: documents of one query with bit-identical feature rows score exactly alike under every
// weight vector, so the reference orders them by its tie-break alone.  gkey[p] = class | group << cls_bits rides in the
// low mantissa bits of the NDCG@k verify kernel's keys (kernels_verify.inc): two close keys of ONE group are an exact
// tie whose order the class bits already give.  Group ids are per query, 1.., 0 = no duplicate.
struct DupGroups {
    // (two bytes per document: the kernel runs with <= 256 classes = 8 bits, and class + group bits are capped at 16)
    std::vector<uint16_t> gkey16;
    uint32_t key_bits = 0, key_cls_bits = 0;
    uint64_t dup_groups = 0;  // groups found, over all queries (whether or not gkey carries their ids)
    int verify_xs = 1;        // keys beyond K the first trainer's verify lists start with
};
// row_hash[p]: a 64-bit hash of position p's feature row (equal rows must hash alike; collisions are sorted out here by
// comparing the rows).  no_dup_groups: FR_NO_DUP_GROUPS.  Queries are strided over nthreads threads.
inline DupGroups duplicate_groups(const std::vector<uint64_t>& row_hash, const HostCSR& csr, const std::vector<uint32_t>& perm_host,
                                  const std::vector<uint32_t>& qstart, const std::vector<uint32_t>& qlen, const std::vector<uint32_t>& gcls,
                                  size_t cls_gain_count, bool no_dup_groups, size_t nthreads) {
    DupGroups out;
    const size_t np = perm_host.size(), nq = qlen.size();
    std::vector<uint32_t> gkey(gcls);
    uint32_t cls_bits = 0;
    while ((size_t(1) << cls_bits) < std::max<size_t>(cls_gain_count, 1)) cls_bits++;
    std::vector<uint32_t> dup(np, 0);
    std::vector<uint32_t> tmax(nthreads, 0);
    std::vector<uint64_t> tsum(nthreads, 0);
    std::vector<char> tmixed(nthreads, 0);  // some group holds documents of different gain classes
    const size_t row_bytes = csr.d * sizeof(float);
    auto work = [&](size_t tid) {
        std::vector<std::pair<uint64_t, uint32_t>> hk;
        for (size_t q = tid; q < nq; q += nthreads) {
            const uint32_t n = qlen[q];
            if (n < 2) continue;
            hk.clear();
            for (uint32_t k = 0; k < n; k++) hk.emplace_back(row_hash[(size_t)qstart[q] + k], k);
            std::sort(hk.begin(), hk.end());
            uint32_t next_id = 1;
            for (size_t i = 0; i < hk.size();) {
                size_t e = i + 1;
                while (e < hk.size() && hk[e].first == hk[i].first) e++;
                if (e - i >= 2) {  // equal hashes: confirm by comparing the rows (sub-groups on a collision)
                    std::vector<char> done(e - i, 0);
                    for (size_t u = i; u < e; u++) {
                        if (done[u - i]) continue;
                        const float* ru = csr.x + (size_t)perm_host[(size_t)qstart[q] + hk[u].second] * csr.d;
                        uint32_t members = 1;
                        for (size_t v = u + 1; v < e; v++) {
                            if (done[v - i]) continue;
                            const float* rv = csr.x + (size_t)perm_host[(size_t)qstart[q] + hk[v].second] * csr.d;
                            if (std::memcmp(ru, rv, row_bytes) == 0) {
                                if (gcls[(size_t)qstart[q] + hk[v].second] != gcls[(size_t)qstart[q] + hk[u].second]) tmixed[tid] = 1;
                                dup[(size_t)qstart[q] + hk[v].second] = next_id;
                                done[v - i] = 1;
                                members++;
                            }
                        }
                        if (members > 1) dup[(size_t)qstart[q] + hk[u].second] = next_id++;
                    }
                }
                i = e;
            }
            tmax[tid] = std::max(tmax[tid], next_id - 1);
            tsum[tid] += next_id - 1;
        }
    };
    std::vector<std::thread> pool;
    for (size_t tid = 1; tid < nthreads; tid++) pool.emplace_back(work, tid);
    work(0);
    for (auto& th : pool) th.join();
    uint32_t maxg = 0;
    for (uint32_t v : tmax) maxg = std::max(maxg, v);
    for (uint64_t v : tsum) out.dup_groups += v;
    uint32_t dup_bits = 0;
    while ((1u << dup_bits) <= maxg) dup_bits++;  // ids 0..maxg
    bool mixed = false;
    for (char v : tmixed) mixed = mixed || v;
    if (!mixed || no_dup_groups) dup_bits = 0;  // (groups of one gain class are covered by the class rule)
    if (cls_bits + dup_bits > 16) dup_bits = cls_bits < 16 ? 16 - cls_bits : 0;  // keep the keys' error term small: late groups lose their id
    out.key_bits = cls_bits + dup_bits;
    out.key_cls_bits = cls_bits;
    if (dup_bits)
        for (size_t p = 0; p < np; p++)
            if (dup[p] && dup[p] < (1u << dup_bits)) gkey[p] |= dup[p] << cls_bits;
    // Where the first trainer on this dataset starts with the length of the verify kernel's lists.  At K + 1 keys a
    // dataset with duplicated rows sends 85 % of the pairs of its first line search to the exact kernel, 16 % of the second
    // (K + 2) and 1.4 % of the third (K + 3) before the lists reach the length the data needs -- 80 ms at the 30K shape, 5 % of
    // a whole job (tools/chain_by_tick.py).  More than half a percent of the documents having an exact duplicate inside
    // their query says so in advance: start at K + 3 (resident_reserve hands a new trainer one below verify_xs; a longer
    // list than the data needs costs ~4 % per key and is never shortened within a trainer, so not K + 4 outright).
    size_t dup_docs = 0;
    for (size_t p = 0; p < np; p++) dup_docs += dup[p] != 0;
    if (dup_docs * 200 > csr.n) out.verify_xs = 4;
    out.gkey16.resize(np);
    for (size_t p = 0; p < np; p++) out.gkey16[p] = (uint16_t)gkey[p];
    return out;
}

// A host stand-in for row_hash_kernel (FNV-1a over the row's bytes), for callers without a device: any hash that maps
// equal rows to equal values gives the same groups.
inline std::vector<uint64_t> host_row_hash(const HostCSR& csr, const std::vector<uint32_t>& perm_host) {
    std::vector<uint64_t> h(perm_host.size(), 0);
    for (size_t p = 0; p < perm_host.size(); p++) {
        if (perm_host[p] == NO_DOCUMENT) continue;
        const unsigned char* row = reinterpret_cast<const unsigned char*>(csr.x + (size_t)perm_host[p] * csr.d);
        uint64_t v = 0xcbf29ce484222325ull;
        for (size_t b = 0; b < csr.d * sizeof(float); b++) v = (v ^ row[b]) * 0x100000001b3ull;
        h[p] = v;
    }
    return h;
}

}  // namespace frdev
