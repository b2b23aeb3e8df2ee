// csrc/lambdamart_goss.hpp run on its own under -fsanitize=address,undefined (tests/test_lambdamart_goss_host.py builds and
// runs this): the key stream, the uniform and the plan of the two rates at their edges -- lists of 0, 1 and 2^32 - 1 entries,
// rates at the ends of their ranges, the largest instance id -- with the properties that follow from the definition
// ("GOSS") checked on the way.
#include "lambdamart_goss.hpp"

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

int main() {
    const uint64_t seeds[] = {0, 1, 0x8000000000000000ull, 0xFFFFFFFFFFFFFFFFull, GOSS_STREAM};
    for (uint64_t seed : seeds) {
        // the stream is Rand64(seed ^ GOSS_STREAM) read in order, and of_tree(t) is its t-th value
        GossKeys keys(seed);
        Rand64 same(seed ^ GOSS_STREAM), master(seed);
        for (uint32_t t = 0; t < 40; t++) {
            const uint64_t k = keys.next();
            CHECK(k == same.rand_u64());
            if (t < 6) CHECK(GossKeys::of_tree(seed, t) == k);
        }
        // ... and not the per-tree samples' (a seed equal to the stream constant aside, whose stream is Rand64(0))
        if (seed != GOSS_STREAM) CHECK(GossKeys::of_tree(seed, 0) != master.rand_u64());
        // the uniform: in [0, 1), a function of (key, id) alone, also at the ends of the id range
        const uint64_t key = GossKeys::of_tree(seed, 3);
        const uint32_t ids[] = {0u, 1u, 63u, 0x7FFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu};
        for (uint32_t id : ids) {
            const double u = goss_uniform(key, id);
            CHECK(u >= 0.0 && u < 1.0 && u == goss_uniform(key, id));
            CHECK(u * 0x1.0p53 == (double)(uint64_t)(u * 0x1.0p53));  // 53 bits
        }
        CHECK(goss_uniform(key, 0) != goss_uniform(key, 1) && goss_uniform(key, 0) != goss_uniform(key + 1, 0));
    }
    // the plan: n_top follows sample_count (at least 1 of a non-empty list, never more than the list); a + b = 1 keeps everything
    const size_t lens[] = {0, 1, 2, 7, 1000, 3800000, 0xFFFFFFFFull};
    const double tops[] = {1e-300, 0.1, 0.2, 0.5, 0.75, 1.0 - 0x1.0p-53};
    for (size_t n : lens) {
        for (double a : tops) {
            const GossPlan p = goss_plan(n, a, 0.1 <= 1.0 - a ? 0.1 : 1.0 - a);
            CHECK(p.n_top == sample_count(n, a) && p.n_top <= n && (n == 0 || p.n_top >= 1));
            CHECK(p.p > 0.0 && p.amp > 0.0);
        }
    }
    const double halves[][2] = {{0.5, 0.5}, {0.25, 0.75}, {0.75, 0.25}, {0.125, 0.875}};
    for (const auto& h : halves) {
        const GossPlan p = goss_plan(1000, h[0], h[1]);
        CHECK(p.p == 1.0 && p.amp == 1.0);
    }
    const GossPlan usual = goss_plan(1000, 0.2, 0.1);
    CHECK(usual.n_top == 200 && usual.p == 0.1 / (1.0 - 0.2) && usual.amp == (1.0 - 0.2) / 0.1 && usual.amp > 1.0);
    std::printf("lambdamart_goss ok\n");
    return 0;
}
