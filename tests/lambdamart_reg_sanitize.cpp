// csrc/lambdamart_reg.hpp run on its own under -fsanitize=address,undefined (tests/test_lambdamart_reg_host.py builds and runs
// this): the designed cases of the leaf regularisation ("Leaf regularisation") -- a gradient sum exactly at
// the threshold, a zero sum, a zero denominator, an output exactly at the cap, a path_smooth so large that r + 1.0 rounds to
// 1.0 and one so small that r is huge, bounds that bind before and after smoothing, the largest integer sums -- with the
// properties that follow from the definition checked on the way.
#include "lambdamart_reg.hpp"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

using namespace fr;

#define CHECK(...)                                                                 \
    do {                                                                           \
        if (!(__VA_ARGS__)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    const HistReg off{};
    CHECK(!off.on() && HistReg{0.5, 0.0, 0.0}.on() && HistReg{0.0, 1.0, 0.0}.on() && HistReg{0.0, 0.0, 2.0}.on());
    // nothing set: the Newton leaf and term, bit for bit (s_l = s_w = 4: G = q / 16, H = w / 16)
    {
        const RegSide s = reg_side(48, 32, 7, 4, 4, 1.0, off, nullptr, -inf, inf);
        CHECK(s.v == 3.0 / 3.0 && s.term == (3.0 * 3.0) / 3.0);
    }
    // |G| == l1 exactly, and below it: the thresholded sum, the output and the term are all 0
    for (long long q : {48ll, -48ll, 16ll, 0ll}) {
        const RegSide s = reg_side(q, 32, 7, 4, 4, 1.0, HistReg{3.0, 0.0, 0.0}, nullptr, -inf, inf);
        CHECK(s.v == 0.0 && s.term == 0.0);
    }
    // ... and above it the sign is kept
    CHECK(reg_side(64, 32, 7, 4, 4, 1.0, HistReg{3.0, 0.0, 0.0}, nullptr, -inf, inf).v == 1.0 / 3.0);
    CHECK(reg_side(-64, 32, 7, 4, 4, 1.0, HistReg{3.0, 0.0, 0.0}, nullptr, -inf, inf).v == -1.0 / 3.0);
    // a zero denominator: the leaf rule's 0.0
    CHECK(reg_side(48, 0, 7, 4, 4, 0.0, HistReg{0.0, 5.0, 0.0}, nullptr, -inf, inf).v == 0.0);
    // an output exactly at the cap stays where it is and keeps the plain term; beyond it, it is moved
    {
        const HistReg cap{0.0, 1.0, 0.0};
        const RegSide at = reg_side(48, 32, 7, 4, 4, 1.0, cap, nullptr, -inf, inf);
        CHECK(at.v == 1.0 && at.term == 3.0);
        const RegSide over = reg_side(96, 32, 7, 4, 4, 1.0, cap, nullptr, -inf, inf), under = reg_side(-96, 32, 7, 4, 4, 1.0, cap, nullptr, -inf, inf);
        CHECK(over.v == 1.0 && over.term == (2.0 * 6.0) * 1.0 - (3.0 * 1.0) * 1.0);
        CHECK(under.v == -1.0 && under.term == over.term);
        // a tiny hessian sum: the quotient overflows to +inf and is capped
        const RegSide tiny = reg_side(0x7000000000000000ll, 1, 7, -900, 1000, 0.0, cap, nullptr, -inf, inf);
        CHECK(tiny.v == 1.0);
    }
    // smoothing: the root is not pulled; a huge path_smooth (r + 1.0 == 1.0) gives the parent's output, a tiny one (r huge)
    // leaves the child's own
    {
        const double parent = -2.0;
        CHECK(reg_side(48, 32, 7, 4, 4, 1.0, HistReg{0.0, 0.0, 4.0}, nullptr, -inf, inf).v == 1.0);
        const RegSide mid = reg_side(48, 32, 4, 4, 4, 1.0, HistReg{0.0, 0.0, 4.0}, &parent, -inf, inf);  // r = 1
        CHECK(mid.v == (1.0 * 1.0) / 2.0 + -2.0 / 2.0 && mid.term == (2.0 * 3.0) * mid.v - (3.0 * mid.v) * mid.v);
        const RegSide all = reg_side(48, 32, 1, 4, 4, 1.0, HistReg{0.0, 0.0, 0x1.0p60}, &parent, -inf, inf);
        CHECK(all.v == (1.0 * 0x1.0p-60) / 1.0 + -2.0 / 1.0);
        const RegSide none = reg_side(48, 32, 0xFFFFFFFFu, 4, 4, 1.0, HistReg{0.0, 0.0, 0x1.0p-900}, &parent, -inf, inf);
        CHECK(none.v == 1.0 && none.term == 3.0);
    }
    // bounds: one that binds before smoothing and no longer after it, and one that binds only after it
    {
        const double parent = -2.0;
        const HistReg sm{0.0, 0.0, 4.0};
        CHECK(reg_side(48, 32, 4, 4, 4, 1.0, off, nullptr, -inf, 0.5).v == 0.5);
        CHECK(reg_side(48, 32, 4, 4, 4, 1.0, sm, &parent, -inf, 0.5).v == -0.5);
        CHECK(reg_side(48, 32, 4, 4, 4, 1.0, off, nullptr, 0.0, inf).v == 1.0);
        const RegSide held = reg_side(48, 32, 4, 4, 4, 1.0, sm, &parent, 0.0, inf);
        CHECK(held.v == 0.0 && held.term == 0.0);
    }
    // a node's own term at a carried output: the plain one where the output is its own quotient
    CHECK(reg_own_term(48, 32, 4, 4, 1.0, off, 1.0) == 3.0 && reg_own_term(48, 32, 4, 4, 1.0, off, 0.5) == (2.0 * 3.0) * 0.5 - (3.0 * 0.5) * 0.5);
    // the ends of the integer range and of the exponents: finite or not, nothing traps
    const long long ends[] = {std::numeric_limits<long long>::min(), -1, 0, 1, std::numeric_limits<long long>::max()};
    double sink = 0.0;
    for (long long q : ends)
        for (long long w : ends)
            for (int s : {-1074, -60, 0, 61, 1100})
                for (const HistReg& r : {off, HistReg{1.0, 1.0, 1.0}, HistReg{0x1.0p-1074, 1e300, 1e308}}) {
                    const double parent = 0.25;
                    const RegSide a = reg_side(q, w, 0u, s, s, 0.0, r, &parent, -1.0, 1.0);
                    CHECK(a.v != a.v || (a.v >= -1.0 && a.v <= 1.0));
                    sink += a.v == a.v ? a.v : 0.0;
                }
    std::printf("lambdamart_reg ok (%g)\n", sink);
    return 0;
}
