// The three encodings of a forest that the scoring kernels read, packed on the host: no HIP in this
// header.  score_trees.inc uploads what these functions return and launches; permute.inc takes the adjacent-children layout;
// fr_debug_forest_pack (capi.cpp) hands the packed tables to the CPU tests (tests/test_forest_pack_host.py decodes them
// with tests/forest_pack_model.py; tests/forest_pack_sanitize.cpp runs the packers at their limits under the sanitizers).
//   pack_forest_rank          tree_ensemble_rank_kernel (kernels_treerank.inc): Eytzinger threshold tables, ranking rounds, heap-shaped
//                             batches with u16 leaf ids
//   pack_forest_lds           tree_ensemble_lds_kernel (kernels_tree.inc): breadth-first 8-byte node words with 8-bit child offsets, for
//                             one block shape
//   adjacent_children_layout  tree_ensemble_kernel (the L2 walk) and permute_trees_kernel
// A packer that returns false has found the forest outside one of its encoding's limits; the caller tries the next encoding.
// The packers read no environment: the timing switches of a -DFR_PRICING build arrive in ForestPackOptions.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "device.hpp"  // FlatTrees

namespace frdev {

struct TreeNodeDev {
    double split;  // threshold, or the leaf value when fid < 0
    int32_t fid;   // < 0: leaf
    int32_t lhs;   // left child; the right child is lhs + 1 (children are stored adjacently)
};

// (walks per thread, levels) of every batch of a descriptor list {start, n, levels, ..} x nbatch + terminator
inline std::vector<std::pair<uint32_t, uint32_t>> tree_plan_batches(const std::vector<uint32_t>& desc) {
    std::vector<std::pair<uint32_t, uint32_t>> out;
    for (size_t b = 0; b + 1 < desc.size() / 4; b++) out.emplace_back(desc[b * 4 + 1], desc[b * 4 + 2]);
    return out;
}

// Largest f32 <= split: (f64(x) <= split) <=> (x <= thr) for every non-NaN f32 x.
inline float floor_to_f32(double split) {
    float t = (float)split;
    if ((double)t > split) t = std::nextafterf(t, -std::numeric_limits<float>::infinity());
    return t;
}

// Block shapes of tree_ensemble_lds_kernel: DOCS documents x H parts, PF 16-byte prefetch words
// per thread (x2 batches in flight; bounds the batch size), NMAX walks per thread.
struct TreeShape {
    unsigned docs, parts, pf, nmax;
};
inline constexpr TreeShape TREE_SHAPES[] = {
    {256, 1, 6, 16}, {256, 2, 3, 16}, {256, 4, 4, 8}, {192, 2, 8, 16}, {192, 4, 4, 16}, {128, 1, 24, 16}, {128, 2, 24, 16},
    {128, 4, 12, 16}, {64, 1, 24, 16}, {64, 4, 24, 16},
};
// The (docs, parts) the LDS walk tries, in order of measured speed at the 30K shape (tools/ab/treeshapes.sh, 500 trees: 192 x 4 parts
// 5.4 ms (8 walks per thread), 192 x 2 6.9, 128 x 4 7.4, 256 x 2 7.8); smaller blocks leave more LDS for big trees.
inline constexpr unsigned TREE_ORDER_MULTI[][2] = {{192, 4}, {192, 2}, {128, 4}, {256, 2}, {256, 4}, {128, 2}, {64, 4}};
// a single-tree model returns the bare leaf (no 0.0 + 1.0 * leaf), which only one-part blocks do
inline constexpr unsigned TREE_ORDER_SINGLE[][2] = {{256, 1}, {128, 1}, {64, 1}};

// Block shape of tree_ensemble_rank_kernel: the launcher's template arguments and the packer's arithmetic.
struct RankBlock {
    static constexpr unsigned DOCS = 192, H = 4, PF = 2;
};

// What the packers took from the environment of a -DFR_PRICING build (the timing experiments of device.hpp's third kind
// of switch); the defaults are "unset", which is all the shipped library knows.
struct ForestPackOptions {
    int cap_kb = -1;       // FR_TREE_CAP_KB: caps the LDS walk's batch area (< 0: unset)
    int nmax = 0;          // FR_TREE_NMAX: caps the walks per thread, >= 1 (0: unset)
    bool nowalk = false;   // FR_TREE_NOWALK: every batch walks 0 levels (staging + batch streaming only)
    bool nostage = false;  // FR_TREE_NOSTAGE: no ranking rounds (garbage codes, same walk cost)
};

// tree_ensemble_lds_kernel's buffers for one block shape (layout: kernels_tree.inc)
struct LdsForest {
    std::vector<uint64_t> forest;  // the batches' 8-byte words, every batch padded to a multiple of two
    std::vector<uint32_t> desc;    // {offset (16-byte units), N, levels, 0} x nbatch + terminator
    std::vector<double> leafprod;  // [0] = +0.0: the padding trees' product
    size_t lds_bytes = 0;
};

// tree_ensemble_rank_kernel's buffers (layout: kernels_treerank.inc)
struct RankForest {
    std::vector<uint32_t> fdesc, rdesc;
    std::vector<float> tables;
    std::vector<uint32_t> forest, desc;  // forest: 32-bit words, every batch a multiple of 16 bytes; desc: {offset (16-byte units), N, L, leafbase}
    std::vector<double> leafprod;
    uint32_t nslots = 0, nrounds = 0;
    size_t lds_bytes = 0;
};

// Packs the forest for one block shape of tree_ensemble_lds_kernel (layout: see kernels_tree.inc).  false: the forest does
// not fit the compact encoding in this shape.
inline bool pack_forest_lds(const FlatTrees& t, const TreeShape& sh, uint32_t d, uint32_t dq, const ForestPackOptions& opt, LdsForest* out) {
    const TreeShape* shape = &sh;
    const size_t nt = t.root.size();
    const uint32_t pad_slot = (uint32_t)dq * 4;  // the 0.0 slot that follows the feature columns in LDS
    if (nt == 0) return false;
    const size_t lds_cap = 160 * 1024;
    const size_t fixed_bytes = ((size_t)shape->docs * (dq * 4 + 1) * sizeof(float) + 15) / 16 * 16 +
                               (shape->parts > 1 ? (size_t)shape->docs * 8 : 0);
    if (fixed_bytes + 8 * 1024 > lds_cap) return false;
    size_t tree_bytes_cap = std::min<size_t>((size_t)shape->pf * 16 * shape->docs * shape->parts, (lds_cap - fixed_bytes) / 16 * 16);
    if (opt.cap_kb >= 0) tree_bytes_cap = std::min<size_t>(tree_bytes_cap, opt.cap_kb * 1024);
    size_t H = shape->parts, max_n = shape->nmax;
    if (opt.nmax) max_n = std::max(1, std::min((int)max_n, opt.nmax));  // (benchmarking)
    const uint32_t slot_bytes = shape->docs * 4, pad_off = pad_slot * slot_bytes;  // node words carry LDS byte offsets
    const size_t words_cap = tree_bytes_cap / 8;
    struct Packed {
        std::vector<uint64_t> words;  // node words (indices relative to the tree's first word); a leaf's lo32 = index of
        uint32_t nodes = 0, levels = 0;  // its product in `leafprod`
    };
    std::vector<double>& leafprod = out->leafprod;
    leafprod.assign(1, 0.0);  // [0] = +0.0: the padding trees' product
    std::vector<double> tw = t.weight;
    tw.resize(nt, 1.0);
    std::vector<Packed> packed(nt + 1);  // [nt] = the padding tree: one leaf, product +0.0
    for (size_t k = 0; k <= nt; k++) {
        Packed& pk = packed[k];
        std::vector<uint64_t> nodes;
        const double w = k < nt ? tw[k] : 0.0;
        if (k == nt) {
            nodes.push_back((uint64_t)pad_off << 32);  // product index 0
        } else {
            struct Item { int32_t src; uint32_t dst; uint32_t depth; };
            std::vector<Item> work;  // FIFO: breadth-first, so one level's nodes are contiguous in LDS and
            nodes.push_back(0);      // the lanes of a wave (all on the same level) spread over the banks
            work.push_back({t.root[k], 0u, 0u});
            for (size_t head = 0; head < work.size(); head++) {
                const Item it = work[head];
                pk.levels = std::max(pk.levels, it.depth);
                if (t.fid[it.src] < 0) {
                    if (leafprod.size() >= (size_t(1) << 23)) return false;  // the index rides in an f32's bits as a small non-negative number
                    nodes[it.dst] = ((uint64_t)pad_off << 32) | (uint64_t)leafprod.size();
                    // out += weight * leaf (src/model.rs:104-112): the product does not depend on the document
                    leafprod.push_back(t.raw_single ? t.split[it.src] : w * t.split[it.src]);
                } else {
                    const uint32_t left = (uint32_t)nodes.size();
                    const uint32_t rel = left - it.dst;
                    if (rel > 0xFF || nodes.size() + 2 > words_cap) return false;  // rel is 8 bits (a level of <= 255 nodes)
                    const uint32_t slot = ((uint32_t)t.fid[it.src] < d ? (uint32_t)t.fid[it.src] : pad_slot) * slot_bytes;
                    float thr = floor_to_f32(t.split[it.src]);
                    uint32_t tb;
                    std::memcpy(&tb, &thr, 4);
                    nodes[it.dst] = ((uint64_t)rel << 56) | ((uint64_t)slot << 32) | tb;
                    nodes.push_back(0);
                    nodes.push_back(0);
                    work.push_back({t.lhs[it.src], left, it.depth + 1});
                    work.push_back({t.rhs[it.src], left + 1, it.depth + 1});
                }
            }
        }
        pk.nodes = (uint32_t)nodes.size();
        pk.words = std::move(nodes);
        if (pk.words.size() + 1 + (H - 1) * 2 > words_cap) return false;  // must fit beside H-1 padding trees
    }
    // Cut into batches of H*N trees, N the largest of 16/8/4/2/1 whose trees fit; when not even H
    // trees fit (or fewer than H remain) the batch is N = 1 with padding trees.
    std::vector<uint64_t>& forest = out->forest;
    std::vector<uint32_t>& desc = out->desc;
    forest.clear(), desc.clear();
    size_t k0 = 0;
    while (k0 < nt) {
        std::vector<size_t> members;  // tree ids; nt = padding
        size_t n = 0;
        for (size_t cand = max_n; cand >= 1 && n == 0; cand /= 2) {
            if (k0 + H * cand > nt) continue;
            size_t words = 0;
            for (size_t k = k0; k < k0 + H * cand; k++) words += packed[k].words.size() + 1;
            if (words <= words_cap) n = cand;
        }
        if (n > 0) {
            for (size_t k = k0; k < k0 + H * n; k++) members.push_back(k);
        } else {
            n = 1;
            size_t words = H * 2;  // as if all padding (a padding tree is 1 word + 1 header word)
            for (size_t k = k0; k < nt && members.size() < H; k++) {
                if (words - 2 + packed[k].words.size() + 1 > words_cap) break;
                words += packed[k].words.size() + 1 - 2;
                members.push_back(k);
            }
            while (members.size() < H) members.push_back(nt);
        }
        const size_t ntb = members.size(), start = forest.size();
        uint32_t levels = 0;
        desc.insert(desc.end(), {(uint32_t)(start / 2), (uint32_t)n, 0u, 0u});
        forest.resize(start + ntb);
        for (size_t i = 0; i < ntb; i++) {
            const size_t k = members[i];
            const std::vector<uint64_t>& words = packed[k].words;
            forest[start + i] = (uint32_t)(forest.size() - start);  // root
            forest.insert(forest.end(), words.begin(), words.end());
            levels = std::max(levels, packed[k].levels);
            if (k < nt) k0 = k + 1;
        }
        desc[desc.size() - 2] = opt.nowalk ? 0u : levels;
        if (forest.size() & 1) forest.push_back(0);
    }
    desc.insert(desc.end(), {(uint32_t)(forest.size() / 2), 0u, 0u, 0u});
    out->lds_bytes = fixed_bytes + words_cap * 8;
    return true;
}

// FNV-1a over a forest's nodes, roots and weights: the key of the packed-forest cache (never 0)
inline uint64_t forest_hash(const FlatTrees& t) {
    uint64_t hash = 0xcbf29ce484222325ull;
    {
        auto mix = [&](const void* p, size_t bytes) {
            const uint64_t* w = (const uint64_t*)p;
            for (size_t i = 0; i < bytes / 8; i++) hash = (hash ^ w[i]) * 0x100000001b3ull;
            const unsigned char* b = (const unsigned char*)p + bytes / 8 * 8;
            for (size_t i = 0; i < bytes % 8; i++) hash = (hash ^ b[i]) * 0x100000001b3ull;
        };
        mix(t.fid.data(), t.fid.size() * sizeof(int32_t));
        mix(t.lhs.data(), t.lhs.size() * sizeof(int32_t));
        mix(t.rhs.data(), t.rhs.size() * sizeof(int32_t));
        mix(t.split.data(), t.split.size() * sizeof(double));
        mix(t.root.data(), t.root.size() * sizeof(int32_t));
        mix(t.weight.data(), t.weight.size() * sizeof(double));
        const uint64_t shape[2] = {t.fid.size(), t.root.size()};
        mix(shape, sizeof(shape));
        if (hash == 0) hash = 1;
    }
    return hash;
}

// Packs the forest for tree_ensemble_rank_kernel (kernels_treerank.inc: threshold ranks instead of features).  false: the
// forest does not fit that encoding: a single bare tree (raw output), a leaf deeper
// than 10 levels, more than 1023 distinct thresholds on one feature, or more than 170 features in use (85 pairs of u16 codes
// x 768 bytes + the two constant codes end at 65282 < 2^16).
inline bool pack_forest_rank(const FlatTrees& t, uint32_t d, uint32_t dq, const ForestPackOptions& opt, RankForest* out) {
    const size_t nt = t.root.size();
    if (nt == 0 || t.raw_single) return false;
    constexpr unsigned DOCS = RankBlock::DOCS, H = RankBlock::H, PF = RankBlock::PF;
    constexpr size_t area_bytes = (size_t)PF * 16 * DOCS * H;  // batch area = what two prefetch slots of a block carry
    const size_t nf = (size_t)dq * 4;

    // ---- distinct thresholds per feature, as f32 (largest f32 <= split), -0.0 folded onto +0.0
    std::vector<std::vector<float>> thr(nf);
    for (size_t i = 0; i < t.fid.size(); i++) {
        if (t.fid[i] < 0 || (uint32_t)t.fid[i] >= d) continue;
        float v = floor_to_f32(t.split[i]);
        if (v != v) continue;  // NaN threshold: the node always goes right
        if (v == 0.0f) v = 0.0f;
        thr[(size_t)t.fid[i]].push_back(v);
    }
    std::vector<uint32_t>& fdesc = out->fdesc;
    fdesc.assign(nf * 4, 0u);
    std::vector<uint32_t> slotoff(nf, 0xFFFFFFFFu);
    std::vector<float>& tables = out->tables;
    tables.clear();
    uint32_t nslots = 0;
    for (size_t f = 0; f < nf; f++) {
        std::vector<float>& v = thr[f];
        fdesc[f * 4] = 0xFFFFFFFFu;
        if (v.empty()) continue;
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        uint32_t logp = 1;
        while ((size_t(1) << logp) <= v.size()) logp++;  // P = 2^logp > count
        if (logp > 10) return false;
        const uint32_t P = 1u << logp;
        slotoff[f] = (nslots >> 1) * DOCS * 4 + (nslots & 1) * 2;  // half (slot & 1) of word slot / 2 of the document's column
        fdesc[f * 4 + 0] = slotoff[f];
        fdesc[f * 4 + 2] = logp;
        fdesc[f * 4 + 3] = P;
        nslots++;
    }
    if ((((size_t)nslots + 1) >> 1) * DOCS * 4 + 2 > 0xFFFF) return false;  // slot offsets ride in 16 bits
    const uint32_t off_p0 = (nslots >> 1) * DOCS * 4 + (nslots & 1) * 2, off_p1 = ((nslots + 1) >> 1) * DOCS * 4 + ((nslots + 1) & 1) * 2;
    // Ranking rounds (see the kernel): part h of a round ranks features of float4 group row * H + h; a group's tables go
    // into as few chunks of <= 8 * DOCS floats as they need (one, unless several of its features have > 255 thresholds),
    // a row of H groups takes as many rounds as its largest group.  Table = Eytzinger order: node i = 2^k + j (level
    // k) holds the sorted element (2j + 1) * P / 2^(k+1) - 1, +inf where there is none.
    constexpr uint32_t chunk_cap = 8 * DOCS;
    static_assert((size_t)H * chunk_cap * 4 <= area_bytes, "the parts' table areas share the batch area");
    std::vector<uint32_t>& rdesc = out->rdesc;
    rdesc.clear();
    for (size_t row = 0; row * H < dq; row++) {
        struct Sub { uint32_t len = 0; uint32_t off[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}; };
        std::vector<Sub> subs[H];
        size_t nsub = 1;
        for (size_t h = 0; h < H; h++) {
            const size_t j4 = row * H + h;
            if (j4 >= dq) continue;
            for (size_t c = 0; c < 4; c++) {
                const size_t f = j4 * 4 + c;
                if (thr[f].empty()) continue;
                const uint32_t P = fdesc[f * 4 + 3];
                if (subs[h].empty() || subs[h].back().len + P > chunk_cap) subs[h].emplace_back();
                subs[h].back().off[c] = subs[h].back().len;
                subs[h].back().len += P;
            }
            nsub = std::max(nsub, subs[h].size());
        }
        for (size_t sub = 0; sub < nsub; sub++)
            for (size_t h = 0; h < H; h++) {
                const size_t j4 = row * H + h;
                if (sub >= subs[h].size()) {
                    rdesc.insert(rdesc.end(), {0u, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu});
                    continue;
                }
                const Sub& sb = subs[h][sub];
                const size_t base = tables.size();
                const uint32_t padded_len = (sb.len + DOCS - 1) / DOCS * DOCS;  // whole rows of DOCS floats (<= chunk_cap), +inf beyond the tables
                tables.resize(base + padded_len, std::numeric_limits<float>::infinity());
                for (size_t c = 0; c < 4; c++) {
                    if (sb.off[c] == 0xFFFFFFFFu) continue;
                    const size_t f = j4 * 4 + c;
                    const std::vector<float>& v = thr[f];
                    const uint32_t logp = fdesc[f * 4 + 2], P = fdesc[f * 4 + 3];
                    for (uint32_t k = 0; k < logp; k++)
                        for (uint32_t j = 0; j < (1u << k); j++) {
                            const size_t idx = (size_t)(2 * j + 1) * (P >> (k + 1)) - 1;
                            if (idx < v.size()) tables[base + sb.off[c] + (1u << k) + j] = v[idx];
                        }
                }
                // the round's features by table depth, deepest first, absent ones last (the kernel's search loops
                // run 1, 2, 3, 4 interleaved chains that end together)
                uint32_t order[4] = {0, 1, 2, 3};
                auto depth_of = [&](uint32_t c) { return sb.off[c] == 0xFFFFFFFFu ? 0u : fdesc[(j4 * 4 + c) * 4 + 2]; };
                std::stable_sort(order, order + 4, [&](uint32_t a, uint32_t b) { return depth_of(a) > depth_of(b); });
                uint32_t flags = sub == 0 ? 1u : 0u;
                for (uint32_t j = 0; j < 4; j++) flags |= order[j] << (8 + 2 * j);
                rdesc.insert(rdesc.end(), {(uint32_t)base, padded_len, (uint32_t)j4, flags, sb.off[order[0]], sb.off[order[1]], sb.off[order[2]], sb.off[order[3]]});
            }
    }
    uint32_t nrounds = (uint32_t)(rdesc.size() / (8 * H));
    if (opt.nostage) nrounds = 0;  // (timing experiments: garbage codes, same walk cost)
    const size_t codes_bytes = (((size_t)nslots + 3) / 2 * DOCS * 4 + 15) / 16 * 16;
    const size_t lds = codes_bytes + (size_t)DOCS * 8 + area_bytes;

    // ---- depth of every tree (steps that surely reach a leaf)
    std::vector<uint32_t> depth(nt, 0);
    {
        std::vector<std::pair<int32_t, uint32_t>> work;
        for (size_t k = 0; k < nt; k++) {
            work.assign(1, {t.root[k], 0u});
            while (!work.empty()) {
                auto [src, dd] = work.back();
                work.pop_back();
                if (t.fid[src] < 0) {
                    depth[k] = std::max(depth[k], dd);
                } else {
                    if (dd >= 10) return false;
                    work.emplace_back(t.lhs[src], dd + 1);
                    work.emplace_back(t.rhs[src], dd + 1);
                }
            }
        }
    }
    std::vector<double> tw = t.weight;
    tw.resize(nt, 1.0);
    size_t max_n = 8;
    if (opt.nmax) max_n = std::max(1, std::min(8, opt.nmax));  // (benchmarking)

    // ---- batches of H*N trees laid out as heaps of the batch's depth
    std::vector<uint32_t>& forest = out->forest;  // forest: 32-bit words, every batch a multiple of 16 bytes
    std::vector<uint32_t>& desc = out->desc;
    std::vector<double>& leafprod = out->leafprod;
    forest.clear(), desc.clear(), leafprod.clear();
    auto node_word = [&](int32_t src) -> uint32_t {
        const uint32_t f = (uint32_t)t.fid[src];
        const float v0 = floor_to_f32(t.split[src]);
        if (v0 != v0) return off_p1;                                 // x <= NaN is false: right
        if (f >= d) return (0.0f <= v0) ? off_p0 : off_p1;           // the feature reads 0.0
        const float v = v0 == 0.0f ? 0.0f : v0;
        const std::vector<float>& tv = thr[f];
        const uint32_t j = (uint32_t)(std::lower_bound(tv.begin(), tv.end(), v) - tv.begin());
        return (j << 16) | slotoff[f];
    };
    size_t k0 = 0;
    while (k0 < nt) {
        size_t n = 0, count = 0;
        uint32_t L = 1;
        for (size_t cand = max_n; cand >= 1 && n == 0; cand /= 2) {
            if (k0 + H * cand > nt) continue;
            uint32_t l = 1;
            for (size_t k = k0; k < k0 + H * cand; k++) l = std::max(l, depth[k]);
            if (H * cand * (size_t(6) << l) <= area_bytes) n = cand, L = l, count = H * cand;
        }
        if (n == 0) {  // fewer than H trees left, or deep trees: one walk per part, padding trees fill the parts
            n = 1;
            for (size_t k = k0; k < nt && count < H; k++) {
                const uint32_t l = std::max(L, depth[k]);
                if (H * (size_t(6) << l) > area_bytes) break;
                L = l;
                count++;
            }
            if (count == 0) return false;
        }
        const size_t start = forest.size(), leafbase = leafprod.size();
        const size_t tw_words = (size_t(6) << L) / 4, bottom = size_t(1) << L;
        desc.insert(desc.end(), {(uint32_t)(start / 4), (uint32_t)n, L, (uint32_t)leafbase});
        if (opt.nowalk) desc[desc.size() - 2] = 0;  // (timing experiments: staging + batch streaming only)
        forest.resize(start + (H * n * tw_words + 3) / 4 * 4, 0u);
        leafprod.push_back(0.0);  // id 0: the padding trees' product, +0.0
        for (size_t i = 0; i < H * n; i++) {
            uint32_t* nodes = forest.data() + start + i * tw_words;
            uint16_t* ids = (uint16_t*)(nodes + bottom);
            for (size_t h = 0; h < bottom; h++) nodes[h] = off_p0;  // "stay left": code 0 > 0 is false
            for (size_t h = 0; h < bottom; h++) ids[h] = 0;
            if (i >= count) continue;
            const size_t k = k0 + i;
            struct Item { int32_t src; uint32_t h, dd; };
            std::vector<Item> work(1, Item{t.root[k], 1u, 0u});
            while (!work.empty()) {
                const Item it = work.back();
                work.pop_back();
                if (t.fid[it.src] < 0) {
                    const size_t id = leafprod.size() - leafbase;
                    if (id > 0xFFFF) return false;
                    leafprod.push_back(tw[k] * t.split[it.src]);  // out += weight * leaf (src/model.rs:104-112)
                    const size_t span = size_t(1) << (L - it.dd), first = ((size_t)it.h << (L - it.dd)) - bottom;
                    for (size_t b = 0; b < span; b++) ids[first + b] = (uint16_t)id;
                } else {
                    nodes[it.h] = node_word(it.src);
                    work.push_back(Item{t.lhs[it.src], 2 * it.h, it.dd + 1});
                    work.push_back(Item{t.rhs[it.src], 2 * it.h + 1, it.dd + 1});
                }
            }
        }
        k0 += count;
    }
    desc.insert(desc.end(), {(uint32_t)(forest.size() / 4), 0u, 0u, 0u});
    out->nslots = nslots, out->nrounds = nrounds, out->lds_bytes = lds;
    return true;
}

// The forest re-laid so that the two children of a node are adjacent (rhs = lhs + 1): what tree_ensemble_kernel and
// permute_trees_kernel walk.  A tree's nodes are contiguous, from roots[k] to the next tree's root.
inline void adjacent_children_layout(const FlatTrees& t, std::vector<TreeNodeDev>& nodes, std::vector<int32_t>& roots) {
    const size_t nt = t.root.size();
    nodes.clear();
    roots.assign(nt, 0);
    nodes.reserve(t.fid.size() + nt);
    {
        std::vector<std::pair<int32_t, int32_t>> work;  // (source node, destination slot)
        for (size_t k = 0; k < nt; k++) {
            roots[k] = (int32_t)nodes.size();
            nodes.push_back(TreeNodeDev{0.0, -1, 0});
            work.emplace_back(t.root[k], roots[k]);
            while (!work.empty()) {
                auto [src, dst] = work.back();
                work.pop_back();
                nodes[dst].split = t.split[src];
                nodes[dst].fid = t.fid[src];
                nodes[dst].lhs = 0;
                if (t.fid[src] >= 0) {
                    int32_t kids = (int32_t)nodes.size();
                    nodes[dst].lhs = kids;
                    nodes.push_back(TreeNodeDev{0.0, -1, 0});
                    nodes.push_back(TreeNodeDev{0.0, -1, 0});
                    work.emplace_back(t.lhs[src], kids);
                    work.emplace_back(t.rhs[src], kids + 1);
                }
            }
        }
    }
}

}  // namespace frdev
