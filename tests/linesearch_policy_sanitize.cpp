// csrc/linesearch_policy.hpp run on its own under -fsanitize=address,undefined (tests/test_device_form_host.py builds and runs
// this): every policy driven with scripted observations.  The expected sequences are worked out by hand from the
// transitions as the line-search driver made them before they moved into the header (commit 30d7be4, device_dataset.inc:
// ls_submit's routing block and rank-planning loop, topk_policy, ls_collect); each derivation stands next to its checks.
#include "linesearch_policy.hpp"

#include <cstdio>
#include <cstdlib>

using namespace frdev;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

// one line search of verify groups on the given slots; returns the refresh entries written
struct Tick {
    int32_t buf[16];  // entry[0..G) | entry_group[0..G), as in the tick block (o_rank)
    size_t n = 0;
};
static Tick rank_tick(LsPolicy& p, const std::vector<long>& gslot, const std::vector<char>& upd, unsigned period, const std::vector<uint8_t>& half) {
    Tick t;
    const size_t G = gslot.size();
    for (int32_t& v : t.buf) v = -7;
    t.n = p.plan_rank_refresh(G, [&](size_t g) { return (size_t)gslot[g]; }, [&](size_t g) { return upd[g] != 0; }, period, half, t.buf, t.buf + G);
    return t;
}

static void test_refresh_schedule() {
    const std::vector<uint8_t> half = {0, 1, 0};
    LsPolicy p;
    p.reset(3);
    // An update on every line search, period 16.  Fresh: age = 0xFFFF, gap = 1.
    //   LS 1: age == 0xFFFF -> refresh; the gap doubles only where age != 0xFFFF, so it stays 1; age = 1.
    //   LS 2: age 1 >= min(16, gap 1), upd > 0 -> refresh; gap 2; age = 1.
    //   LS 3: age 1 < 2 -> age 2.  LS 4: 2 >= 2 -> refresh; gap 4.  LS 5-7: age 2, 3, 4.  LS 8: 4 >= 4 -> refresh; gap 8.
    //   LS 9-15: age 2..8.  LS 16: 8 >= 8 -> refresh; gap 16.  LS 17-31: age 2..16.  LS 32: 16 >= 16 -> refresh; gap 32.
    //   From here min(period, gap) = 16: LS 33-47 age 2..16, LS 48 refresh (gap 64), LS 64 refresh.
    std::vector<int> at;
    for (int ls = 1; ls <= 70; ls++) {
        const Tick t = rank_tick(p, {1}, {1}, 16, half);
        if (t.n) {
            CHECK(t.n == 1 && t.buf[0] == 1 * 2 + 1 && t.buf[1] == 0);  // slot * 2 + half, the group
            at.push_back(ls);
        }
    }
    CHECK((at == std::vector<int>{1, 2, 4, 8, 16, 32, 48, 64}));
    CHECK(p.slots[1].rank_gap == 128 && p.slots[1].rank_age == 7 && p.slots[1].rank_upd == 6);  // LS 65-70: age 2..7, six updates waiting
    // A shorter period caps the gap's effect, not the gap: period 3 -> 1, 2, 4 (gap 4 -> min 3), then every 3: 7, 10, 13
    p.reset(3);
    at.clear();
    for (int ls = 1; ls <= 14; ls++)
        if (rank_tick(p, {0}, {1}, 3, half).n) at.push_back(ls);
    CHECK((at == std::vector<int>{1, 2, 4, 7, 10, 13}));
    // No updates: a fresh slot still refreshes at its first line search (age == 0xFFFF needs no update); after it upd stays 0,
    // so nothing refreshes, age rises by one per line search and stops at 0xFFFE (0xFFFF means "never made")
    p.reset(3);
    CHECK(rank_tick(p, {2}, {0}, 16, half).n == 1);
    CHECK(p.slots[2].rank_age == 1 && p.slots[2].rank_gap == 1);
    for (int ls = 0; ls < 70000; ls++) CHECK(rank_tick(p, {2}, {0}, 16, half).n == 0);
    CHECK(p.slots[2].rank_age == 0xFFFE && p.slots[2].rank_upd == 0);
    // ... and one update then refreshes at once (age >= gap 1), the gap starts doubling
    CHECK(rank_tick(p, {2}, {1}, 16, half).n == 1 && p.slots[2].rank_gap == 2 && p.slots[2].rank_age == 1);
    // new_sums: age = 0xFFFF, gap = 1 -> the next line search refreshes without an update and leaves the gap at 1
    for (int ls = 0; ls < 5; ls++) rank_tick(p, {2}, {1}, 16, half);  // (age 2, refresh and gap 4, age 2, 3, 4)
    CHECK(p.slots[2].rank_gap == 4 && p.slots[2].rank_age == 4);
    p.new_sums(2);
    p.new_sums(99);  // (out of range: ignored)
    CHECK(p.slots[2].rank_age == 0xFFFF && p.slots[2].rank_gap == 1);
    CHECK(rank_tick(p, {2}, {0}, 16, half).n == 1 && p.slots[2].rank_gap == 1 && p.slots[2].rank_age == 1);
    CHECK(rank_tick(p, {2}, {1}, 16, half).n == 1 && p.slots[2].rank_gap == 2);  // 1, 2, 4, ... again
    // mode 2: never listed, nothing moves; a group without a slot (-1 -> out of range) is passed over
    p.reset(3);
    p.slots[0].rank_mode = 2;
    for (int ls = 0; ls < 40; ls++) CHECK(rank_tick(p, {0, -1}, {1, 1}, 16, half).n == 0);
    CHECK(p.slots[0].rank_age == 0xFFFF && p.slots[0].rank_upd == 0 && p.slots[0].rank_gap == 1);
}

static void test_two_groups_on_one_slot() {
    // A restart with more than 64 candidates: groups 0 and 2 on slot 1, group 1 on slot 0, all fresh, all with an update.
    //   g0: upd 1, age 0xFFFF -> entry (1*2+0, group 0), upd 0.  g1: entry (0*2+1, group 1).  g2: upd 1, age is still 0xFFFF
    //   (ages are written behind the loop) -> due again, but slot 1 is listed: no entry, group 2 not recorded; upd 0.
    const std::vector<uint8_t> half = {1, 0};
    LsPolicy p;
    p.reset(2);
    const Tick t = rank_tick(p, {1, 0, 1}, {1, 1, 1}, 16, half);
    CHECK(t.n == 2 && t.buf[0] == 2 && t.buf[1] == 1 && t.buf[2] == -7);
    CHECK(t.buf[3] == 0 && t.buf[4] == 1 && t.buf[5] == -7);
    CHECK(p.slots[1].rank_age == 1 && p.slots[1].rank_upd == 0 && p.slots[1].rank_gap == 1);
    // routing: both groups of slot 1 go to the exact kernel, its counter goes down ONCE (first loop marks on exact_left > 0
    // without touching it, second loop decrements per distinct slot)
    p.slots[1].exact_left = 2;
    const std::vector<long> gslot = {1, 0, 1};
    CHECK(p.route(3, [&](size_t g) { return gslot[g]; }) == 2);
    CHECK(p.routed[0] == 1 && p.routed[1] == 0 && p.routed[2] == 1);
    CHECK(p.slots[1].exact_left == 1 && p.slots[0].exact_left == 0 && p.exact_groups == 2);
}

static void chain(LsPolicy& p, long slot, unsigned runs, double t_off = RANK_OFF_BELOW, double t_on = RANK_ON_ABOVE) {
    // two groups of the slot, 1000 documents each: runs / 2000 per visit
    p.observe_chain(3, [&](size_t k) { return k == 1 ? -1L : slot; }, [&](size_t k) { return k == 1 ? 999999u : runs / 2; }, 1000, t_off, t_on);
}

static void test_mode_switch() {
    LsPolicy p;
    p.reset(2);
    // 15 observations of 0 runs: rate_n 1..15 < 16 -> no decision however low the mean.  The 16th: n = 16, mean 0 < 0.16 -> off.
    for (int i = 0; i < 15; i++) chain(p, 0, 0);
    CHECK(p.slots[0].rank_mode == 1 && p.slots[0].rate_n == 15 && p.rank_slots_off == 0);
    chain(p, 0, 0);
    CHECK(p.slots[0].rank_mode == 2 && p.rank_slots_off == 1 && p.rank_slots_on == 0);
    CHECK(p.slots[1].rate_n == 0);  // (a slot without a group in the tick is not observed; the group without a slot is passed over)
    // 0.18 per visit from here: the mean climbs from 0 towards 0.18 by sixteenths, never past 0.21 -> stays off
    for (int i = 0; i < 200; i++) chain(p, 0, 360);
    CHECK(p.slots[0].rank_mode == 2 && p.slots[0].rate > 0.17f && p.slots[0].rate < 0.181f && p.rank_slots_off == 1 && p.rank_slots_on == 0);
    // 0.5 per visit: mean ~0.18 + 0.32/16 = 0.20 (not above 0.21), then 0.20 + 0.30/16 = 0.219 -> on at the second observation
    chain(p, 0, 1000);
    CHECK(p.slots[0].rank_mode == 2);
    chain(p, 0, 1000);
    CHECK(p.slots[0].rank_mode == 1 && p.rank_slots_on == 1 && p.rank_slots_off == 1);
    // a slot that is on and whose mean lies between the thresholds stays on: 16 and more observations of exactly 0.18
    for (int i = 0; i < 40; i++) chain(p, 1, 360);
    CHECK(p.slots[1].rank_mode == 1 && p.slots[1].rate_n == 16 && p.rank_slots_on == 1 && p.rank_slots_off == 1);
    // the thresholds are the caller's: with off-below 0.2 the same mean switches off
    chain(p, 1, 360, 0.2, 0.3);
    CHECK(p.slots[1].rank_mode == 2 && p.rank_slots_off == 2);
}

// verify groups on the given slots with the given redone pairs, of nq = 100 pairs each
static void redo(LsPolicy& p, const std::vector<long>& gslot, const std::vector<uint32_t>& n, int xs_used, int cap, bool pinned, int debug, int& xs,
                 size_t nq = 100) {
    p.observe_redo(gslot.size(), [&](size_t k) { return gslot[k]; }, [&](size_t k) { return n[k]; }, nq, xs_used, cap, pinned, debug, xs);
}

static void test_backoff() {
    LsPolicy p;
    p.reset(3);
    int xs = 1;
    // pinned length -> the verdict branch.  Failing = redone * 4 > nq: 26 of 100 fails, 25 does not.
    //   failing: backoff = min(16, max(4, backoff * 2)): 0 -> 4 -> 8 -> 16 -> 16, exact_left = backoff each time
    const unsigned want[4] = {4, 8, 16, 16};
    for (int i = 0; i < 4; i++) {
        redo(p, {0}, {26}, 1, 4, true, 0, xs);
        CHECK(p.slots[0].backoff == want[i] && p.slots[0].exact_left == want[i]);
    }
    redo(p, {1}, {26}, 1, 4, true, 0, xs);  // slot 1 fails once; slot 0 is not seen in this tick
    CHECK(p.slots[1].backoff == 4 && p.slots[1].exact_left == 4 && p.slots[0].backoff == 16 && p.slots[0].exact_left == 16);
    //   succeeding: backoff /= 2: 16 -> 8 -> 4 -> 2 -> 1 -> 0 -> 0; exact_left is the router's to count down, slot 1 untouched
    const unsigned down[6] = {8, 4, 2, 1, 0, 0};
    for (int i = 0; i < 6; i++) {
        redo(p, {0, -1}, {25, 99}, 1, 4, true, 0, xs);
        CHECK(p.slots[0].backoff == down[i] && p.slots[0].exact_left == 16);
    }
    CHECK(p.slots[1].backoff == 4 && p.slots[1].exact_left == 4 && p.slots[2].backoff == 0 && xs == 1);
    // two groups of one slot, one of them failing: the slot fails
    redo(p, {2, 2}, {0, 30}, 1, 4, true, 0, xs);
    CHECK(p.slots[2].backoff == 4 && p.slots[2].exact_left == 4);
    // a timing ablation (debug != 0) takes no verdict
    redo(p, {2}, {30}, 1, 4, true, 1, xs);
    CHECK(p.slots[2].backoff == 4);
    // routing consumes exact_left, one per tick, and reports the groups routed; a group that is not the owner's (-1) stays
    const std::vector<long> gslot = {1, -1, 0};
    p.slots[0].exact_left = 0;
    for (int i = 0; i < 4; i++) {
        CHECK(p.route(3, [&](size_t g) { return gslot[g]; }) == 1 && p.routed[0] == 1 && p.routed[1] == 0 && p.routed[2] == 0);
        CHECK(p.slots[1].exact_left == 3 - i);
    }
    CHECK(p.route(3, [&](size_t g) { return gslot[g]; }) == 0 && p.routed[0] == 0 && p.exact_groups == 4);
    // a new trainer starts without back-off; the statistics run on
    p.reset(2);
    CHECK(p.slots.size() == 2 && p.slots[1].backoff == 0 && p.slots[1].exact_left == 0 && p.slots[1].rank_age == 0xFFFF && p.exact_groups == 4);
}

static void test_list_length_ramp() {
    CHECK(verify_xs_cap(1) == 3 && verify_xs_cap(5) == 3 && verify_xs_cap(6) == 4 && verify_xs_cap(10) == 4 && verify_xs_cap(20) == 4 && VERIFY_XS_MAX == 4);
    LsPolicy p;
    p.reset(1);
    int xs = 1;
    // nq = 1000, two groups: raised when total * 250 > 2000, i.e. total >= 9.  Group 1's 300 redone pairs would be a failing
    // verdict (1200 > 1000): on a tick that raises the length none is taken (either / or)
    redo(p, {0, 0}, {4, 4}, 1, 4, false, 0, xs, 1000);  // total 8: not raised -> verdict branch, succeeding
    CHECK(xs == 1 && p.slots[0].backoff == 0);
    redo(p, {0, 0}, {5, 4}, 1, 4, false, 0, xs, 1000);  // total 9
    CHECK(xs == 2 && p.slots[0].backoff == 0);
    redo(p, {0, 0}, {5, 300}, 2, 4, false, 0, xs, 1000);
    CHECK(xs == 3 && p.slots[0].backoff == 0);
    redo(p, {0, 0}, {5, 300}, 1, 4, false, 0, xs, 1000);  // a launch still in flight with the old length: already higher, stays; no verdict
    CHECK(xs == 3 && p.slots[0].backoff == 0);
    redo(p, {0, 0}, {5, 300}, 3, 3, false, 0, xs, 1000);  // depth <= 5: the cap of 3 is reached -> the verdict
    CHECK(xs == 3 && p.slots[0].backoff == 4 && p.slots[0].exact_left == 4);
    redo(p, {0, 0}, {5, 300}, 3, 4, false, 0, xs, 1000);  // deeper: one more key
    CHECK(xs == 4 && p.slots[0].backoff == 4);
    redo(p, {0, 0}, {5, 300}, 4, 4, false, 0, xs, 1000);  // the longest lists: the verdict
    CHECK(xs == 4 && p.slots[0].backoff == 8);
    xs = 1;
    redo(p, {0, 0}, {5, 300}, 1, 4, true, 0, xs, 1000);  // pinned: never raised, the verdict
    CHECK(xs == 1 && p.slots[0].backoff == 16);
}

static void test_redo_grid() {
    // times 4 above half the grid used (strictly), from at least 512, up to 8192
    CHECK(next_redo_grid(512, 512, 256) == 512 && next_redo_grid(512, 512, 257) == 2048);
    CHECK(next_redo_grid(2048, 2048, 1025) == 8192 && next_redo_grid(8192, 8192, 8000) == 8192 && next_redo_grid(4096, 4096, 4000) == 8192);
    CHECK(next_redo_grid(64, 64, 33) == 2048);
    // halved below a sixteenth (strictly), never below 512
    CHECK(next_redo_grid(2048, 2048, 127) == 1024 && next_redo_grid(2048, 2048, 128) == 2048);
    CHECK(next_redo_grid(1024, 1024, 0) == 512 && next_redo_grid(512, 512, 0) == 512);
    // the grid USED decides (a pinned launch), the context's own grid is what moves
    CHECK(next_redo_grid(512, 4096, 100) == 512 && next_redo_grid(2048, 64, 33) == 8192 && next_redo_grid(2048, 4096, 255) == 1024);
}

static void test_skip_and_threshold() {
    LsPolicy p;
    CHECK(!p.take_skip());
    p.observe_skip(50, 100, 2);  // 200 > 200: no
    CHECK(p.approx_skip == 0);
    p.observe_skip(51, 100, 2);
    CHECK(p.approx_skip == 16);
    for (int i = 0; i < 16; i++) CHECK(p.take_skip());
    CHECK(!p.take_skip() && p.approx_skip == 0);
    p.reset(4);  // (the counter is the dataset's, not a trainer's)
    p.observe_skip(51, 100, 2);
    p.reset(4);
    CHECK(p.approx_skip == 16);
    // kappa * sqrt(sum (w_j sigma_j)^2) / sigma_f: (1.5 * 2, 4 * 1) -> 5; / 2 * 0.5 = 1.25.  A constant column: no threshold
    CHECK(order_threshold({1.5, 4.0}, {2.0, 1.0}, 0, 0.5) == 1.25 && order_threshold({1.5, 4.0}, {2.0, 1.0}, 1, 1.0) == 5.0);
    CHECK(std::isinf(order_threshold({1.5, 4.0}, {2.0, 0.0}, 1, 1.0)));
}

int main() {
    test_refresh_schedule();
    test_two_groups_on_one_slot();
    test_mode_switch();
    test_backoff();
    test_list_length_ramp();
    test_redo_grid();
    test_skip_and_threshold();
    std::printf("linesearch_policy ok\n");
    return 0;
}
