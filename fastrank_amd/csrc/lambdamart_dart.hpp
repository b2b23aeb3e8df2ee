// LambdaMART's DART boosting ("DART"): which earlier trees a tree is fitted without, and how the
// ensemble's weights change when it is added.  Host arithmetic only, no device: the trainer (lambdamart.hpp) and the debug
// hook fr_debug_lambdamart_dart_plan replay it, tests/lambdamart_dart_sanitize.cpp runs it under the sanitizers.
//
// The state before tree t (0-based) is the weights w_0 .. w_{t-1} (f64).
//   plan      its own generator Rand64(seed ^ DART_STREAM), read with rand_float() only, so the per-tree sample seeds drawn
//             from Rand64(seed) are untouched.  Tree 0 draws nothing and drops nothing.  Tree t >= 1 draws exactly 1 + t
//             floats, u then c_0 .. c_{t-1}, whatever the rates: the stream position of a tree depends on t alone.
//             u < skip_drop: D_t is empty.  Otherwise D_t = {i : c_i < drop_rate}, cut to its max_drop smallest indices when
//             max_drop > 0.  An empty D_t is an ordinary boosting step (no drop is forced).
//   weights   k = |D_t|: w_t = learning_rate / (double)(k + 1); for i in D_t w_i = w_i * f with f = (double)k / (double)(k + 1)
//             rounded first.  k = 0 gives w_t = learning_rate exactly and touches nothing else.
#pragma once
#include <cstdint>
#include <vector>

#include "host.hpp"

namespace fr {

constexpr uint64_t DART_STREAM = 0x4441525444415254ull;  // "DARTDART"

class DartPlan {
  public:
    DartPlan(uint64_t seed, double drop_rate, uint32_t max_drop, double skip_drop)
        : gen_(seed ^ DART_STREAM), drop_rate_(drop_rate), skip_drop_(skip_drop), max_drop_(max_drop) {}
    // D_t, ascending; to be called for t = 0, 1, 2, ... in order
    std::vector<uint32_t> next(uint32_t t) {
        std::vector<uint32_t> dropped;
        if (t == 0) return dropped;
        const bool skip = gen_.rand_float() < skip_drop_;
        for (uint32_t i = 0; i < t; i++) {
            const double c = gen_.rand_float();  // (drawn also when the tree skips its drop or the cap is reached)
            if (!skip && c < drop_rate_ && (max_drop_ == 0 || dropped.size() < (size_t)max_drop_)) dropped.push_back(i);
        }
        return dropped;
    }

  private:
    Rand64 gen_;
    double drop_rate_, skip_drop_;
    uint32_t max_drop_;
};

// w_0 .. w_{t-1} -> w_0 .. w_t after a tree that was fitted without the trees `dropped`
inline void dart_reweight(std::vector<double>& w, const std::vector<uint32_t>& dropped, double learning_rate) {
    const double k = (double)dropped.size();
    const double f = k / (k + 1.0);
    for (uint32_t i : dropped) w[i] = w[i] * f;
    w.push_back(learning_rate / (k + 1.0));
}

// the trees a re-forming of the scores covers: 0 .. t-1 without `dropped` (ascending)
inline std::vector<uint32_t> dart_kept(uint32_t t, const std::vector<uint32_t>& dropped) {
    std::vector<uint32_t> kept;
    size_t d = 0;
    for (uint32_t i = 0; i < t; i++) {
        if (d < dropped.size() && dropped[d] == i) d++;
        else kept.push_back(i);
    }
    return kept;
}

}  // namespace fr
