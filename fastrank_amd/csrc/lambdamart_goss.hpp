// LambdaMART's gradient-based one-side sampling, host side ("GOSS"; device side: kernels_goss.inc).
// Pure host code, no device call: the key stream, the uniform of a document, and what the two rates turn into.
//
//   key       tree t's key K_t is the t-th rand_u64() of Rand64(seed ^ GOSS_STREAM): a stream of its own, so the per-tree
//             samples (Rand64(seed)), the DART plan (seed ^ DART_STREAM) and the listwise objective's keys (seed ^ XENDCG_STREAM)
//             do not move.
//   uniform   u = (mix(K_t + 0x9E3779B97F4A7C15 (id + 1)) >> 11) 2^-53, mix = the splitmix64 finaliser, id = the document's
//             original instance id: a function of (seed, tree, document) alone, whatever list the document is found in.
//   plan      n_top = sample_count(n_t, top_rate); an other entry is kept iff u < p, p = other_rate / (1.0 - top_rate); the kept
//             others' lambda and w are multiplied by amp = (1.0 - top_rate) / other_rate.  top_rate + other_rate = 1 gives
//             p = amp = 1.0 exactly.
#pragma once
#include <cstdint>

#include "host.hpp"

namespace fr {

constexpr uint64_t GOSS_STREAM = 0x474F5353474F5353ull;  // "GOSSGOSS"

class GossKeys {
  public:
    explicit GossKeys(uint64_t seed) : gen_(seed ^ GOSS_STREAM) {}
    uint64_t next() { return gen_.rand_u64(); }  // K_0, K_1, ...: one per tree, in order
    // K_tree without keeping a stream
    static uint64_t of_tree(uint64_t seed, uint32_t tree) {
        GossKeys k(seed);
        uint64_t out = 0;
        for (uint32_t t = 0; t <= tree; t++) out = k.next();
        return out;
    }

  private:
    Rand64 gen_;
};

inline uint64_t goss_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

inline double goss_uniform(uint64_t key, uint32_t id) {
    return (double)(goss_mix(key + 0x9E3779B97F4A7C15ull * ((uint64_t)id + 1ull)) >> 11) * 0x1.0p-53;
}

// what a tree of n_t instances does under the two rates (0 < top_rate < 1, 0 < other_rate, top_rate + other_rate <= 1)
struct GossPlan {
    uint32_t n_top;
    double p, amp;
};
inline GossPlan goss_plan(size_t n_t, double top_rate, double other_rate) {
    return {(uint32_t)sample_count(n_t, top_rate), other_rate / (1.0 - top_rate), (1.0 - top_rate) / other_rate};
}

}  // namespace fr
