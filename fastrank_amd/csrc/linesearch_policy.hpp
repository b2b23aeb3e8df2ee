// The adaptive policies of the bound-and-verify line search (DESIGN.md sections 4.2 / 4.3): what the device is asked to do on
// the next tick, decided from what the last ticks reported.  State and transitions only -- no HIP and no environment here:
// the driver (device_dataset.inc: ls_submit / ls_collect / topk_policy) reads the switches (FR_RANK_PERIOD, FR_ORDER_KAPPA,
// FR_RANK_OFF_BELOW, FR_RANK_ON_ABOVE, FR_VERIFY_XS) and hands the values in, together with the counts the kernels
// returned.  tests/linesearch_policy_sanitize.cpp drives every transition below without a device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

namespace frdev {

constexpr int VERIFY_XS_MAX = 4;  // the longest lists compiled (K + 4 keys)
// keys beyond K a verify launch of this depth may keep (depth <= 5: K + 3 keys at most)
inline int verify_xs_cap(int64_t depth) { return depth <= 5 ? 3 : VERIFY_XS_MAX; }

// Chain runs per (document, group) visit (running mean of a restart) below which its R ranks stop being refreshed, and above
// which they are again.  Measured (profiles/r06_rank_policy.txt; ranks kept / never made, and what keeping them is worth):
// mslr 0.148 / 0.195 (-1 %), ties 0.177 / 0.225 (+3 %), tiesmix 0.177 / 0.232 (+6 %), hard 0.180 / 0.319 (+12 %), hardties
// 0.209 / 0.362 (+21 %).
constexpr double RANK_OFF_BELOW = 0.16, RANK_ON_ABOVE = 0.21;

// visiting order of the resident verify kernel (kernels_verify.inc): per group the |w_c - base_f| below which a
// candidate ranks like the current model -- where the spread its change of w_f adds, |delta| sigma_x(f), stays under
// the spread of the current scores, sqrt(sum_j (w_j sigma_j)^2)
inline double order_threshold(const std::vector<double>& weights, const std::vector<double>& colstd, size_t feature, double kappa) {
    double var = 0.0;
    for (size_t j = 0; j < colstd.size(); j++) {
        const double t = weights[j] * colstd[j];
        var += t * t;
    }
    const double sx = colstd[feature];
    return sx > 0.0 ? kappa * std::sqrt(var) / sx : std::numeric_limits<double>::infinity();
}

// (the grid follows the redo counts this context has seen, 512 .. 8192 pairs: a short list wants a short grid --
// every block, empty or not, needs a wave slot, and those are contested while another set's verify grid is
// dispatching -- a long one (tie-heavy data) must not cost a second round trip)
// current: the context's grid; used: the grid of the launch the count nredo came from (FR_REDO_GRID may have pinned it)
inline unsigned next_redo_grid(unsigned current, unsigned used, uint32_t nredo) {
    if (nredo > used / 2) return std::min(8192u, std::max(current, 512u) * 4u);
    if (nredo < used / 16 && current > 512u) return current / 2u;
    return current;
}

// The policies of one trainer's restarts (a resident slot = a restart); the statistics they feed count over every trainer the
// dataset has had.
struct LsPolicy {
    struct Slot {
        // NDCG@k: line searches still to be sent straight to the exact kernel, and the length of the current back-off
        // (4, 8, 16: doubled while the verify kernel keeps failing on that restart, halved when it succeeds)
        uint8_t exact_left = 0, backoff = 0;
        uint16_t rank_age = 0xFFFF;  // line searches since the slot's ranks were made (0xFFFF: never)
        uint16_t rank_upd = 0;       // accepted candidates (changes of R) since then
        uint16_t rank_gap = 1;       // line searches until the next refresh: 1, 2, 4, ... up to the period (a young model moves fast)
        // Does keeping a restart's R ranks pay?  The verify kernel counts, per group, the documents that made it run its insertion
        // chain; the host keeps a running mean of that count per (document, group) visit for every restart (its features differ
        // from one line search to the next: the mean is over ~16 of them).  Ranks are made at a restart's first line search -- early
        // in training nothing else orders the documents -- and refreshed every few line searches WHILE the chain runs often enough
        // for the upkeep to pay: a restart whose chain runs rarely even so (storage order is gain descending, and where the
        // labels carry the scores that is nearly R descending already) stops refreshing (mode 2: the last table stays, a stale
        // order only costs admissions) and starts again if the chain runs creep up.  The two thresholds are measured, on five
        // kinds of data (profiles/r06_rank_policy.txt).
        uint8_t rank_mode = 1;  // 1 ranks refreshed, 2 not
        uint16_t rate_n = 0;    // line searches in the running mean
        float rate = 0.0f;      // running mean of chain runs per visit
    };
    std::vector<Slot> slots;
    uint32_t approx_skip = 0;  // MRR / full-ranking paths: ticks for which the exact kernels are used directly (after a tick with many redos)
    unsigned long long exact_groups = 0;                       // NDCG@k: group line searches routed to the exact kernel
    unsigned long long rank_slots_on = 0, rank_slots_off = 0;  // rank-mode decisions made (statistics)
    // (scratch of the calls below, kept for its capacity: one record serves all of a dataset's line-search contexts, whose
    // submits and collects run one at a time under the dataset's mutex)
    std::vector<char> routed;  // route(): per staged group, 1 = the exact kernel takes it
    std::vector<char> mark;    // per slot
    std::vector<double> runs, visits;

    // a new trainer: no back-off; the slots' R-rank tables start as the identity (storage order) and are made on a slot's
    // first line search
    void reset(size_t nslots) { slots.assign(nslots, Slot{}); }

    // (new sums: the old ranks say nothing about them, and a young model moves fast again)
    void new_sums(size_t slot) {
        if (slot < slots.size()) {
            slots[slot].rank_age = 0xFFFF;
            slots[slot].rank_gap = 1;
        }
    }

    // Top-k, per-group routing: a restart whose last verified line search left more than a quarter of its pairs undecided
    // (its weights make many scores tie exactly) sends its next few line searches straight to the exact kernel -- the other
    // groups of the tick stay on the verify kernel.
    // slot_of(g): the resident slot of the caller's group g, or -1 where it is not the owner's.  Marks the groups in `routed`
    // and returns their number.
    template <class SlotOf>
    size_t route(size_t G, SlotOf slot_of) {
        routed.assign(G, 0);
        size_t nE = 0;
        for (size_t g = 0; g < G; g++) {
            const long slot = slot_of(g);
            if (slot >= 0 && (size_t)slot < slots.size() && slots[slot].exact_left > 0) {
                routed[g] = 1;
                nE++;
            }
        }
        if (nE > 0) {
            // (once per distinct slot and tick: a restart with more than 64 candidates has several groups on one slot)
            mark.assign(slots.size(), 0);
            for (size_t g = 0; g < G; g++) {
                if (!routed[g]) continue;
                const size_t slot = (size_t)slot_of(g);
                if (mark[slot]) continue;
                mark[slot] = 1;
                if (slots[slot].exact_left > 0) slots[slot].exact_left--;
            }
            exact_groups += nE;
        }
        return nE;
    }

    // the R ranks of a restart are redone after its first 1, 2, 4, 8 line searches and then every 16 (FR_RANK_PERIOD in a
    // pricing build; a stale order only costs admissions: 16 against 8 is +1.4 % in the first 25 ticks of a job and level
    // afterwards, profiles/r06_rank_policy.txt)
    // group_slot(g) / group_updates(g): the resident slot of verify group g (as size_t: none = out of range) and whether the
    // group carries a pending update; half[slot]: the current half of the slot's sums.  Writes the slots to refresh as
    // entry[k] = slot * 2 + half, k < the number returned, and entry_group[k] = a staged group of that slot.
    template <class GroupSlot, class GroupUpdates>
    size_t plan_rank_refresh(size_t nV, GroupSlot group_slot, GroupUpdates group_updates, unsigned period, const std::vector<uint8_t>& half,
                             int32_t* entry, int32_t* entry_group) {
        size_t nrank = 0;
        for (size_t g = 0; g < nV; g++) {
            const size_t slot = group_slot(g);
            if (slot < slots.size() && slots[slot].rank_mode == 1) {
                Slot& s = slots[slot];
                if (group_updates(g) && s.rank_upd < 0xFFFF) s.rank_upd++;
                // (ranks age only while the sums change: a restart that accepts nothing keeps its order)
                // (a restart's first accepted steps move its model the most: ranks made from the initial sums are stale one line
                // search later -- 0.32-0.34 chain runs per visit through ticks 1-7 of a job against 0.16-0.19 behind the first refresh,
                // tools/chain_by_tick.py -- so the first refreshes come after 1, 2 and 4 line searches, then every `period`)
                if (s.rank_age == 0xFFFF || (s.rank_age >= std::min<unsigned>(period, s.rank_gap) && s.rank_upd > 0)) {
                    bool listed = false;  // (a restart with more than 64 candidates has several groups)
                    for (size_t k = 0; k < nrank; k++) listed = listed || (entry[k] >> 1) == (int32_t)slot;
                    if (!listed) {
                        entry_group[nrank] = (int32_t)g;  // (rslot_kernel applies this group's pending update to the sums it ranks)
                        entry[nrank++] = (int32_t)(slot * 2 + half[slot]);
                    }
                    s.rank_upd = 0;  // (the ranks are made from the sums WITH this tick's pending update applied)
                } else if (s.rank_age < 0xFFFE) {
                    s.rank_age++;
                }
            }
        }
        for (size_t k = 0; k < nrank; k++) {
            Slot& s = slots[(size_t)(entry[k] >> 1)];
            if (s.rank_age != 0xFFFF && s.rank_gap < 0x4000) s.rank_gap *= 2;  // 1, 2, 4, ... line searches to the next refresh
            s.rank_age = 1;
        }
        return nrank;
    }

    // the restarts' running means of chain runs per visit, and the switch (see Slot::rank_mode)
    // slot_of(k): the resident slot of verify group k (-1: none); runs_of(k): its chain runs; every group visited n documents
    template <class SlotOf, class RunsOf>
    void observe_chain(size_t nV, SlotOf slot_of, RunsOf runs_of, size_t n, double t_off, double t_on) {
        runs.assign(slots.size(), 0.0);
        visits.assign(slots.size(), 0.0);
        for (size_t k = 0; k < nV; k++) {
            const long slot = slot_of(k);
            if (slot < 0 || (size_t)slot >= slots.size()) continue;
            runs[slot] += (double)runs_of(k);
            visits[slot] += (double)n;
        }
        for (size_t slot = 0; slot < runs.size(); slot++) {
            if (visits[slot] == 0.0) continue;
            Slot& s = slots[slot];
            const double r = runs[slot] / visits[slot];
            if (s.rate_n < 16) s.rate_n++;
            s.rate += (float)((r - (double)s.rate) / (double)s.rate_n);  // (plain mean up to 16, exponential from there)
            if (s.rate_n < 16) continue;
            if (s.rank_mode == 1 && (double)s.rate < t_off) {
                s.rank_mode = 2;
                rank_slots_off++;
            } else if (s.rank_mode == 2 && (double)s.rate > t_on) {
                s.rank_mode = 1;
                rank_slots_on++;
            }
        }
    }

    // tie-heavy data (more than 0.4 % of the pairs redone -- a redone pair costs ~12 verified ones, a longer list ~4 % of
    // the kernel): first keep more keys per list (up to K + 4), so that tied clusters of one
    // gain class may straddle the cut (raised only; a new trainer starts one below the last one's; launches already in flight used
    // the old length).  With the longest lists (or a pinned length), a restart whose line search still left more than
    // a quarter of its pairs undecided -- its weights make scores tie exactly -- sends its next 4 / 8 / 16 line
    // searches to the exact kernel (doubled while the verify kernel keeps failing on it, halved when it succeeds).
    // slot_of(k) / redo_of(k): the resident slot (-1: none) and the redone pairs of verify group k, of nq pairs each; xs_used,
    // xs_cap, xs_pinned: the list length of that launch, the longest its depth allows, and whether FR_VERIFY_XS chose it;
    // debug: FR_LS_DEBUG (a timing ablation takes no verdict); verify_xs: the dataset's list length
    template <class SlotOf, class RedoOf>
    void observe_redo(size_t nV, SlotOf slot_of, RedoOf redo_of, size_t nq, int xs_used, int xs_cap, bool xs_pinned, int debug, int& verify_xs) {
        size_t total = 0;
        for (size_t k = 0; k < nV; k++) total += redo_of(k);
        if (total * 250 > nq * nV && xs_used < xs_cap && !xs_pinned) {
            if (verify_xs <= xs_used) verify_xs = xs_used + 1;
        } else if (debug == 0) {
            // (per distinct slot: 1 = seen, 2 = one of its groups left more than a quarter of its pairs undecided)
            mark.assign(slots.size(), 0);
            for (size_t k = 0; k < nV; k++) {
                const long slot = slot_of(k);
                if (slot < 0 || (size_t)slot >= slots.size()) continue;
                mark[slot] |= (char)(((size_t)redo_of(k) * 4 > nq) ? 3 : 1);
            }
            for (size_t slot = 0; slot < mark.size(); slot++) {
                Slot& s = slots[slot];
                if (mark[slot] & 2) {
                    s.backoff = (uint8_t)std::min<unsigned>(16u, std::max<unsigned>(4u, s.backoff * 2u));
                    s.exact_left = s.backoff;
                } else if (mark[slot]) {
                    s.backoff = (uint8_t)(s.backoff / 2u);
                }
            }
        }
    }

    // full ranking / reciprocal rank: many pairs redone (more than a quarter of nq * G) -- the exact kernels take the next 16
    // line searches
    void observe_skip(uint32_t nredo, size_t nq, size_t G) {
        if ((size_t)nredo * 4 > nq * G) approx_skip = 16;
    }
    // ... counted down at submit: true = this line search goes to the exact kernels
    bool take_skip() {
        if (approx_skip == 0) return false;
        approx_skip--;
        return true;
    }
};

}  // namespace frdev
