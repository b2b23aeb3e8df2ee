// csrc/lambdamart_dart.hpp run on its own under -fsanitize=address,undefined (tests/test_lambdamart_dart_host.py builds and
// runs this): the drop plan and the re-weighting replayed at their edges -- 1 and 300 trees, rates 0 and 1, max_drop 0, 1 and
// beyond the tree count -- with the properties that follow from the definition ("DART") checked on the way.
#include "lambdamart_dart.hpp"

#include <cstdio>
#include <cstdlib>

using namespace fr;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

struct Replay {
    std::vector<std::vector<uint32_t>> dropped;
    std::vector<double> w;
};

// the trainer's use of the header: plan, the kept list, the re-weighting, tree after tree
static Replay replay(uint64_t seed, double drop_rate, uint32_t max_drop, double skip_drop, uint32_t T, double lr) {
    Replay r;
    DartPlan plan(seed, drop_rate, max_drop, skip_drop);
    for (uint32_t t = 0; t < T; t++) {
        const std::vector<uint32_t> d = plan.next(t);
        CHECK(d.size() <= t && (max_drop == 0 || d.size() <= max_drop));
        for (size_t i = 0; i < d.size(); i++) CHECK(d[i] < t && (i == 0 || d[i] > d[i - 1]));
        const std::vector<uint32_t> kept = dart_kept(t, d);
        CHECK(kept.size() + d.size() == t);
        for (size_t i = 0; i < kept.size(); i++) CHECK(kept[i] < t && (i == 0 || kept[i] > kept[i - 1]));
        const std::vector<double> before = r.w;
        dart_reweight(r.w, d, lr);
        CHECK(r.w.size() == (size_t)t + 1);
        CHECK(r.w[t] == lr / (double)(d.size() + 1));
        for (uint32_t i : kept) CHECK(r.w[i] == before[i]);
        const double f = (double)d.size() / (double)(d.size() + 1);
        for (uint32_t i : d) CHECK(r.w[i] == before[i] * f);
        r.dropped.push_back(d);
    }
    return r;
}

int main() {
    const uint64_t seeds[] = {0, 1, 0x8000000000000000ull, 0xFFFFFFFFFFFFFFFFull, DART_STREAM};
    const uint32_t trees[] = {1, 2, 300};
    const uint32_t caps[] = {0, 1, 50, 1000};
    for (uint64_t seed : seeds) {
        for (uint32_t T : trees) {
            for (uint32_t cap : caps) {
                // rate 0 (what a request without the keys plans) and skip_drop 1: nothing is ever dropped, every weight is lr
                for (const Replay& r : {replay(seed, 0.0, cap, 0.0, T, 0.1), replay(seed, 1.0, cap, 1.0, T, 0.1)}) {
                    for (const auto& d : r.dropped) CHECK(d.empty());
                    for (double w : r.w) CHECK(w == 0.1);
                }
                // rate 1 without skips: every earlier tree up to the cap, the smallest indices
                const Replay all = replay(seed, 1.0, cap, 0.0, T, 0.25);
                for (uint32_t t = 0; t < T; t++) {
                    const uint32_t k = cap == 0 ? t : std::min(t, cap);
                    CHECK(all.dropped[t].size() == k);
                    for (uint32_t i = 0; i < k; i++) CHECK(all.dropped[t][i] == i);
                }
                // in between: the cap cuts the uncapped plan's list and changes nothing else (the draws do not move)
                const Replay free = replay(seed, 0.5, 0, 0.25, T, 0.1), cut = replay(seed, 0.5, cap, 0.25, T, 0.1);
                for (uint32_t t = 0; t < T; t++) {
                    std::vector<uint32_t> head = free.dropped[t];
                    if (cap != 0 && head.size() > cap) head.resize(cap);
                    CHECK(cut.dropped[t] == head);
                }
            }
        }
    }
    // a plan of one tree draws nothing: the generator's first value is still to come
    DartPlan one(5, 0.5, 3, 0.0);
    CHECK(one.next(0).empty());
    std::printf("lambdamart_dart ok\n");
    return 0;
}
