// Permutation importance: the definition, and the interface between the host side (permute_host.hpp,
// compiled into capi.o) and the scoring kernels (kernels_permute.inc + permute.inc, compiled into device.o).  No HIP.
//
// I = the view's instance ids ascending, n = len(I); G, mix = those of resample.hpp; all integer arithmetic mod 2^64.
//   key   = mix(seed + 3 G)            (resample.hpp holds 1 G and 2 G: 3 G is the next free multiple, no collision)
//   key_r = mix(key + (r + 1) G)       repeat r = 0 .. R-1
//   u_i   = mix(key_r + (i + 1) G)     list index i = 0 .. n-1
//   scope "dataset": order = the list indices sorted by (u_i, i) ascending; src_r(I[i]) = I[order[i]]
//   scope "query":   the same keys; the members i_0 < .. < i_{L-1} of each query sorted by (u, i); src_r(I[i_m]) = I[sorted member m]
// One permutation per (seed, r), shared by all features; it depends on neither R nor the features asked for.
//   D_{f,r}: the view with x'[id][f] = x[src_r(id)][f]; every other value, gain, id and query unchanged
//   values[f][r] = the mean over the view's queries of the evaluator on D_{f,r}, in the fixed shape of the mean over queries
//                  (segments of 256 queries); baseline = the same on the view itself
//   scores on D_{f,r} are the reference's: the unfused f64 dot with j ascending; the tree walk with (double)x <= split and
//   out += w_t leaf_t in tree order (the bare leaf for a single DecisionTree); acc = acc + w member for an ensemble
//   report (host, every operation rounded on its own): d_r = baseline - values[f][r]; importance_f = (sum_r d_r in order) / R;
//   std_f = sqrt(sum_r (d_r - importance_f)^2 / (R - 1)), 0.0 for R = 1
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "resample.hpp"

namespace frpermute {

constexpr uint32_t MAX_REPEATS = 64;
constexpr uint32_t ACC = 8;  // repeats one launch of a permute kernel keeps in registers

inline uint64_t stream_key(uint64_t seed) { return frresample::mix(seed + 3ull * frresample::GOLDEN); }
inline uint64_t repeat_key(uint64_t key, uint32_t r) { return frresample::mix(key + (uint64_t)(r + 1) * frresample::GOLDEN); }
inline uint64_t element_key(uint64_t key_r, uint64_t i) { return frresample::mix(key_r + (i + 1) * frresample::GOLDEN); }

}  // namespace frpermute

namespace frdev {

struct FlatTrees;

// One model whose scores on every D_{f,r} of a chunk go into the chunk's slots: weights (Linear, [d]), (fid, dir)
// (SingleFeature) or trees.  A call with `ensemble` adds the members in order, acc = acc + ens_weight * member per slot.
struct PermuteMember {
    enum Kind { LINEAR, SINGLE, TREES } kind = LINEAR;
    const double* weights = nullptr;
    uint32_t fid = 0;
    double dir = 0.0;
    const FlatTrees* trees = nullptr;
    double ens_weight = 1.0;
};

struct PermuteStats {
    bool gather_xcol = false;  // the substitute values came from the column-major copy (else from the tiles)
    bool rows_in_lds = false;
    uint64_t launches_linear = 0, launches_single = 0, launches_trees = 0, launches_axpy = 0;
    double score_ms = 0.0, upload_ms = 0.0;
};

}  // namespace frdev
