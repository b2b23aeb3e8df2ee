// Part of device.hip (single translation unit; see that file's header).  Bound-and-verify NDCG@k line search:
// the kernel that evaluates almost every (run, group) pair of a coordinate-ascent tick.
//
// NDCG@k depends on a candidate's scores only through the ORDER of each query's best documents, so
// the reference's sequentially rounded sums (kernels_linesearch.inc) are needed only where that
// order cannot be proven from cheaper numbers.  Here:
//
// phase S (lane = document): one dot product A = sum_{j != f} x_j * w_j per document, in any
//   association order (FMA, 16-byte loads, eight in flight).  2*D operations per document instead of
//   CT * (D - f).
// phase K (lane = candidate): the tile's documents are visited in order; (A, x_f, gain class) of a
//   document are broadcast (one 16-byte LDS word: both doubles, the class in x_f's lowest mantissa bits), every
//   candidate lane forms its own approximate score
//   s~_c = fma(x_f, w_c, A) and overwrites the lowest mantissa bits with the gain class, so a list
//   entry is a bare 64-bit key and the ordered insertion into the K+1 best keys is a max/min chain.
//   No transpose, no LDS traffic, thresholds always current.
// RESIDENT variant of phase S: the trainer keeps R ~ sum_j x_j * v_j (v = a restart's un-normalised best
//   weights) in HBM; then A = R * (1/norm) - x_f * base_f costs 24 bytes and three operations per document
//   instead of the whole 544-byte row, and an accepted candidate updates R with two FMAs on the next visit
//   (double-buffered, so the groups of a restart never see a half-updated array).  The host accounts for the
//   accumulated rounding of R in eps (LineGroup::resident_err) and refreshes R exactly now and then.
// verification (query end): both s~ and the reference's sum lie within gamma_(D+1) * T of the
//   real-number sum (T = sum_j |x_j w_j|), so |s~ - s| <= eps_c with the per-candidate constant the
//   host computes from per-column max |x| (eps2 = 2 * eps_c, including the class bits).  Two sorted
//   neighbours more than 2*eps apart are in the reference's order, and so is everything above the upper one
//   relative to everything below the lower one.  Neighbours that are closer (near-ties, exact ties --
//   duplicated documents) may come in either order in the reference, which changes DCG@k only if their
//   gain classes differ: so with L = min(depth, n) the value formed from the classes of the first L keys is
//   the reference's iff (i) every close pair inside the first L keys has equal classes -- or is a lone pair of exact
//   duplicates, whose order is the reference's tie-break and known (a cluster of two to four exact duplicates, see the walk below) -- and (ii) the
//   boundary pair (L, L+1) is far apart -- or, with XS > 1 (more keys kept), the pairs (L, L+1) .. (L+m-1, L+m)
//   are close with equal classes and the pair (L+m, L+m+1) is far apart for some m < XS, i.e. the tied cluster
//   that straddles the cut ends within the keys kept.  Otherwise -- ties the reference's gain/id tie-break decides, longer clusters at the cut,
//   non-finite values -- the (query, group) pair is appended to redo_list and the exact kernel
//   recomputes it.  Either way the published value is the reference's bit for bit.

// One document (its 16-byte word W) against every candidate lane of group GI: key = fma(x_f, w_c, A) with the
// class in the low mantissa bits; if some lane's key reaches its (K+1)-th best, sorted insert by an in-place
// min/max chain (payload-free; equal keys are harmless, any tie inside the first L+1 entries fails the
// verification).  Most admitted keys land in the lower half of every list: then the upper half is left alone.
// The insertion chains: one asm statement per half chain (kernels_chain.inc: no wait state between the pairs, no v_min for
// the value that falls off the end) where that form keeps the kernel inside its registers -- K >= 10 without the duplicate-
// group walk; the others (measured by their ISA: the merged form spills 68-140 bytes there) keep one statement per pair.
// Where a key's class (and duplicate-group) bits come from.  With duplicate groups (DUP) the bits are inserted INVERTED into a
// negative sum: a negative double grows smaller as its low mantissa bits grow, so this keeps "larger class id = lower gain
// sorts first" -- the reference's order among documents of one duplicate group (evaluators.rs:34-49) -- on both sides of zero.
// verify_key_sign(hi) = all ones for a negative key; the walk at a query's end takes the bits back out with it.
__device__ __forceinline__ uint32_t verify_key_sign(uint32_t hi) { return (uint32_t)((int32_t)hi >> 31); }
#define VERIFY_BITS_SRC(WZ, VB) (DUP ? ((WZ) ^ verify_key_sign((uint32_t)((VB) >> 32))) : (WZ))
// Two sorted neighbours ka >= kb are in the reference's order if they lie further apart than the sum of their error bounds.
// A key's bound is eps0 / 2 + gamma * |key| (DESIGN.md section 4.2, round 5): the candidate's own term x_f * w_c enters through
// the key's magnitude (|x_f w_c| <= |key| + T_A) instead of through |w_c| times the column's MAXIMUM -- on quantised columns
// the far candidates of a line search (|w_c| ~ 10^6) order documents of equal x_f by the rest of the sum alone, and a bound
// built from the column's outliers swamped exactly those differences (1 % of the pairs redone on the tie kinds, all of them in
// the slices of the extreme candidates).
__device__ __forceinline__ bool verify_far(double ka, double kb, double eps0, double gam) {
    return (ka - kb) > __builtin_fma(gam, __builtin_fabs(ka) + __builtin_fabs(kb), eps0);
}
// Who runs a chain: the whole wave whenever ANY lane admits (a key below a lane's threshold falls through its chain unchanged).
// The per-lane form -- a divergent branch, one to three lanes of 51 executing the chain -- was tried for the power it might
// save (the socket is at its cap, DESIGN.md 4.1) and measured at -1 % (-DVERIFY_ADMIT(C)=(C)): the mask bookkeeping costs what
// the idle lanes save.
#ifndef VERIFY_ADMIT
#define VERIFY_ADMIT(C) (__ballot(C) != 0ull)
#endif
// The chain in THREE parts (round 6; halves before): the list's slots [0, T1), [T1, T2), [T2, KS).  A key that no lane places
// above slot T2 runs the last part only; the top insertion position over a wave's lanes is nearly uniform over the list
// (tools/sim_verify_lanes.py --mode depth), so the expected run is a little shorter than with halves.  Measured +1 % on the
// headline data, level on the tie kinds (profiles/r06_chain_parts_ab.txt); -DVERIFY_CHAIN_PARTS=2 builds the halves.
#ifndef VERIFY_CHAIN_PARTS
#define VERIFY_CHAIN_PARTS 3
#endif
#define VERIFY_PAIRS(GI, LO, HI)                                                                               \
                _Pragma("unroll") for (int m = (LO); m < (HI); m++) {                                          \
                    double down_;                                                                              \
                    asm("v_min_f64 %0, %1, %2\n\tv_max_f64 %1, %1, %2" : "=&v"(down_), "+v"(slot[GI][m]) : "v"(carry_)); \
                    carry_ = down_;                                                                            \
                }
#define VERIFY_CHAINS(GI)                                                                                      \
            constexpr int T1_ = VERIFY_CHAIN_PARTS == 3 ? KS / 3 : 0, T2_ = VERIFY_CHAIN_PARTS == 3 ? (2 * KS) / 3 : KS / 2; \
            if constexpr (K >= 10 && !DUP) {                                                                   \
                if (VERIFY_ADMIT(key_ >= slot[GI][T2_ - 1])) {                                                   \
                    if constexpr (T1_ > 0) {                                                                   \
                        if (VERIFY_ADMIT(key_ >= slot[GI][T1_ > 0 ? T1_ - 1 : 0])) verify_chain<(T1_ > 0 ? T1_ : 2), false, KS, 0>(slot[GI], carry_); \
                    }                                                                                          \
                    verify_chain<T2_ - T1_, false, KS, T1_>(slot[GI], carry_);                                  \
                }                                                                                              \
                verify_chain<KS - T2_, true, KS, T2_>(slot[GI], carry_);                                       \
            } else {                                                                                           \
                if (VERIFY_ADMIT(key_ >= slot[GI][T2_ - 1])) {                                                   \
                    if constexpr (T1_ > 0) {                                                                   \
                        if (VERIFY_ADMIT(key_ >= slot[GI][T1_ > 0 ? T1_ - 1 : 0])) { VERIFY_PAIRS(GI, 0, T1_) }   \
                    }                                                                                          \
                    VERIFY_PAIRS(GI, T1_, T2_)                                                                 \
                }                                                                                              \
                VERIFY_PAIRS(GI, T2_, KS - 1)                                                                  \
                asm("v_max_f64 %0, %0, %1" : "+v"(slot[GI][KS - 1]) : "v"(carry_));                            \
            }
#define VERIFY_VISIT(GI, W)                                                                                    \
    {                                                                                                          \
        const double Ad_ = __longlong_as_double((long long)(((uint64_t)(W).y << 32) | (W).x));                 \
        const double xf_ = __longlong_as_double((long long)(((uint64_t)(W).w << 32) | (W).z));                 \
        const double v_ = __builtin_fma(xf_, cw[GI], Ad_);                                                     \
        if (VERIFY_ADMIT(v_ >= slot[GI][KS - 1])) {                                                              \
            nchain++; /* (uniform: a scalar add) */                                                            \
            /* admission on the bare sum: it differs from the key (class / duplicate-group bits inserted below) by less   \
               than 2^b ulp, which the error bound carries (compute_eps2: a document turned away here has                 \
               key < threshold + 2^b ulp, and the threshold only rises); a lane that enters the chain with a key below    \
               its threshold just drops it again */                                                            \
            const uint64_t vb_ = (uint64_t)__double_as_longlong(v_);                                           \
            uint32_t lo_; /* class bits from the x_f word, the rest from the sum: one bitfield insert */      \
            asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(lo_) : "s"(cls_mask), "v"(VERIFY_BITS_SRC((W).z, vb_)), "v"((uint32_t)vb_)); \
            const double key_ = __longlong_as_double((long long)((vb_ & 0xFFFFFFFF00000000ull) | lo_));        \
            double carry_ = key_;                                                                              \
            VERIFY_CHAINS(GI)                                                                                  \
        }                                                                                                      \
    }

// Filling a query's empty lists (resident walk).  When a query starts, every lane's list holds -inf and the first K + XS
// documents the lane visits are all admitted: K + XS sorted insertions at ~2 (K + XS) instructions each -- a quarter of the
// kernel's vector instructions at the 30K shape (a query has ~120 documents).  Instead the lane takes the keys of its first
// K + XS documents as they come and sorts them once with a sorting network (kernels_fillnet.inc, generated): 38
// compare-exchanges for 11 keys against 11 x ~13.
#define VERIFY_CE(S, i, j)                                                                                     \
    {                                                                                                          \
        double lo_;                                                                                            \
        asm("v_min_f64 %0, %1, %2\n\tv_max_f64 %1, %1, %2" : "=&v"(lo_), "+v"(S[i]) : "v"(S[j]));             \
        S[j] = lo_;                                                                                            \
    }
#include "kernels_fillnet.inc"
template <int KS> __device__ __forceinline__ void verify_fill_sort(double (&s)[KS]) {
    if constexpr (KS == 6) { VERIFY_FILL_SORT_6(s) }
    else if constexpr (KS == 7) { VERIFY_FILL_SORT_7(s) }
    else if constexpr (KS == 8) { VERIFY_FILL_SORT_8(s) }
    else if constexpr (KS == 9) { VERIFY_FILL_SORT_9(s) }
    else if constexpr (KS == 11) { VERIFY_FILL_SORT_11(s) }
    else if constexpr (KS == 12) { VERIFY_FILL_SORT_12(s) }
    else if constexpr (KS == 13) { VERIFY_FILL_SORT_13(s) }
    else if constexpr (KS == 14) { VERIFY_FILL_SORT_14(s) }
    else if constexpr (KS == 21) { VERIFY_FILL_SORT_21(s) }
    else if constexpr (KS == 22) { VERIFY_FILL_SORT_22(s) }
    else if constexpr (KS == 23) { VERIFY_FILL_SORT_23(s) }
    else { static_assert(KS == 24, "verify_fill_sort: no network of this size"); VERIFY_FILL_SORT_24(s) }
}
// the key of a document's word for this lane: fma(x_f, w_c, A) with the class (and duplicate-group) bits of the x_f word
#define VERIFY_KEY(W, OUT)                                                                                     \
    {                                                                                                          \
        const double v_ = __builtin_fma(__longlong_as_double((long long)(((uint64_t)(W).w << 32) | (W).z)), cw[0], \
                                        __longlong_as_double((long long)(((uint64_t)(W).y << 32) | (W).x)));   \
        const uint64_t vb_ = (uint64_t)__double_as_longlong(v_);                                               \
        uint32_t lo_;                                                                                          \
        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(lo_) : "s"(cls_mask), "v"(VERIFY_BITS_SRC((W).z, vb_)), "v"((uint32_t)vb_)); \
        OUT = __longlong_as_double((long long)((vb_ & 0xFFFFFFFF00000000ull) | lo_));                          \
    }

#ifndef VERIFY_LIVE_ONLY
#define VERIFY_LIVE_ONLY(L) (L)
#endif
#ifndef VERIFY_RANK_BARRIER
#define VERIFY_RANK_BARRIER __builtin_amdgcn_sched_barrier(0);
#endif
// Waves per SIMD of the resident variants (one group per wave): lists of up to K + 2 keys at depth <= 10, longer ones, depth 20
// with K + 1 keys, longer ones.  Seven, not eight, since round 5: with the column-major copy and the masked idle lanes in, the
// 72 registers of seven waves (no scratch, no scalar spills read back with v_readlane) beat the eighth wave by 3.4 %.
#ifndef VERIFY_RES_WAVES
#define VERIFY_RES_WAVES 7
#endif
#ifndef VERIFY_RES_WAVES_LONG
#define VERIFY_RES_WAVES_LONG 7
#endif
#ifndef VERIFY_RES_WAVES_20
#define VERIFY_RES_WAVES_20 6
#endif
#ifndef VERIFY_RES_WAVES_20_LONG
#define VERIFY_RES_WAVES_20_LONG 5
#endif

// GW line groups per wave: the tile's feature loads and f32->f64 converts are shared by the groups (phase S is
// otherwise bound by the L2 -> CU traffic of 32 groups re-reading every tile); each group keeps its own
// candidate weights and lists.
// XS = keys kept beyond the K a list needs: 1 decides the cut by a strict gap; 2 / 3 / 4 also let a tied pair / triple / quadruple
// of one gain class straddle it (the host raises XS while many pairs fail -- tie-heavy data -- at ~4 % more
// instructions per document and step).
// DUP: the dataset has duplicate groups with mixed gains (the host knows): the end-of-query walk also decides lone pairs of
// exact duplicates (otherwise that logic is compiled out: ~2 % of the kernel's instructions).
template <int K, int GW, bool RESIDENT, int XS = 1, bool DUP = false>
__global__ __launch_bounds__(WAVE, (RESIDENT && GW == 1) ? (K >= 20 ? (XS > 1 ? VERIFY_RES_WAVES_20_LONG : VERIFY_RES_WAVES_20) : (XS > 2 ? VERIFY_RES_WAVES_LONG : VERIFY_RES_WAVES)) : (GW >= 4 ? 2 : ((K >= 20 && GW == 2) ? 3 : 4)))
void linesearch_verify_kernel(LSArgs a) {
    constexpr int KS = K + XS;
    // The fast query end -- one gap bound per query in front of the exact pair tests, the quotient without the division (both
    // below, "the current query is complete") -- is compiled into the plain K = 10, XS = 1 variants only: the others are at the
    // edge of their registers, and either part moves them over it (measured by their ISA, profiles/verify_query_end_isa.txt:
    // K = 5 loses its eighth wave, K = 20 spills 120 bytes, the XS > 1 and DUP variants read up to 156 more spilled scalars
    // back with v_readlane).  They keep the walk and the division as they were.
    constexpr bool FAST_END = K == 10 && XS == 1 && !DUP;
    // positions staged per step: a 64-document tile of the feature matrix, or (RESIDENT) a walk tile of up to WT positions that
    // holds whole queries where it can (kernels_order.inc), DPL documents per lane in phase S
    constexpr uint32_t VT = RESIDENT ? WT : (uint32_t)WAVE;
    constexpr uint32_t DPL = VT / (uint32_t)WAVE;
    extern __shared__ __attribute__((aligned(16))) double wl[];       // [GW][4*dq] weights, w_f staged as 0
    // per group and document of the tile: A and x_f, both f64 (no convert per visit); the gain class sits in the lowest
    // mantissa bits of x_f (zero in a converted f32; the 2^(cls_bits-52) relative change of the product is part of eps)
    // RESIDENT (one group per wave): TWO copies of the tile's words, each in its own visiting order -- see "visiting order" below
    __shared__ __attribute__((aligned(16))) uint4 pk[RESIDENT ? 2 : GW][VT + 4];
    const uint32_t lane = threadIdx.x;
    // The DCG terms in LDS behind the weights, rank-major: dtab[rank * ts + class], K rows and one more of zeros (ranks past
    // a short query's end read that one).  A query's end reads its K terms with LDS latency instead of K dependent trips
    // to the L2, and a term's address is the class (the key's low bits) plus a per-rank scalar.
    double* const dtab = wl + (RESIDENT ? 0u : (uint32_t)GW * a.dq * 4u);
    const uint32_t ts = a.ncls + 1u;
    for (uint32_t c = lane; c < ts; c += WAVE)
#pragma unroll
        for (int r = 0; r <= K; r++) dtab[(uint32_t)r * ts + c] = (r < K && c < a.ncls) ? a.dcgtab[(size_t)c * LS_KT + r] : 0.0;
    // XCD-aware block -> (run, group bundle) mapping: blocks b, b+8, b+16.. run on one XCD, so all bundles of a
    // run share that XCD's L2 for the run's feature tiles
    const uint32_t nb = (a.G + GW - 1) / GW;
    const uint32_t blk = blockIdx.x;
    const uint32_t xcd = blk & 7u, seq = blk >> 3;
    const uint32_t g0 = (seq % nb) * GW;
    const uint32_t ri = (seq / nb) * 8u + xcd;
    if (ri >= a.nruns) return;
    const uint32_t r = a.run_order[ri];
    uint32_t q = a.run_q0[r];
    const uint32_t q1 = a.run_q1[r];
    const uint32_t pos = a.run_pos[r];
    const uint32_t first_lo = a.run_lo[r];  // (a view of another dataset's tiles may start inside a tile)
    const uint32_t run_end = pos + a.run_docs[r];
    const uint32_t dq = a.dq, dp = a.dq * 4, d = a.d;
    const double NEG_INF = -__builtin_huge_val();
    const uint32_t cls_mask = a.cls_mask;
    uint32_t f[GW];
    bool live[GW], redo[GW], qbad[GW];
    double cw[GW], my_eps2[GW], slot[GW][KS];
    double *rcur[GW], *roth[GW];  // RESIDENT: current / other half of the restart's resident sums
    double r_inv[GW], r_basef[GW], u_inv[GW], u_basef[GW], u_cand[GW];
    bool r_upd[GW];
    uint32_t u_f[GW];
    const double* par_g = nullptr;  // (GW == 1: the group's row of rs_par)
#pragma unroll
    for (int gi = 0; gi < GW; gi++) {
        const uint32_t g = g0 + gi < a.G ? g0 + gi : a.G - 1;  // a ragged last bundle repeats the last group (not published)
        f[gi] = a.gfeat[g];
        live[gi] = (g0 + gi < a.G) && lane < a.gncand[g];
        cw[gi] = a.gcand[(size_t)g * 64 + lane];
        my_eps2[gi] = a.eps2[(size_t)g * 64 + lane];
        redo[gi] = false;
        if constexpr (RESIDENT) {
            const int32_t sl = a.rs_slot[g];
            rcur[gi] = a.res_cur + (size_t)sl * a.np;
            roth[gi] = a.res_cur + (size_t)(sl ^ 1) * a.np;
            const double* par = a.rs_par + (size_t)g * 6;
            par_g = par;
            r_inv[gi] = par[0];
            r_basef[gi] = par[1];
            r_upd[gi] = par[2] != 0.0;
            u_inv[gi] = par[3];
            u_basef[gi] = par[4];
            u_cand[gi] = par[5];
            u_f[gi] = a.rs_updf[g];
        } else {
            const double* __restrict__ w = a.gw + (size_t)g * dp;
            for (uint32_t j = lane; j < dp; j += WAVE) wl[gi * dp + j] = (j < d && j != f[gi]) ? w[j] : 0.0;
        }
#pragma unroll
        for (int m = 0; m < KS; m++) slot[gi][m] = live[gi] ? NEG_INF : __builtin_huge_val();  // idle lanes admit nothing
    }
    // Visiting order (RESIDENT).  The lists do not depend on the order in which a query's documents are visited (a key is a
    // bare 64-bit number, the chain a min/max network; ties are never decided here), but the NUMBER of chain runs does: the
    // chain runs for the whole wave whenever ANY lane admits, and a lane that meets its best documents first admits few.
    // A candidate's key is R/norm + x_f * (w_c - base_f): candidates near the current weight rank like the current model
    // (R), candidates far above it like x_f descending, far below it like x_f ascending.  So every (query, tile) segment is
    // staged twice -- by R descending (rslot: the trainer's ranks of the resident sums, refreshed every few line searches;
    // any order is valid, a stale one only costs admissions) and by x_f descending (xslot: static per feature, made at
    // upload) -- and a lane walks the copy and direction of its class: near / above / below (the x_f copy backwards).  A
    // column whose smallest (largest) value is shared by many documents ranks those by R again: the host then sends the
    // lanes below (above) to the R copy (gmode bits).  No tables (stateless use, FR_VERIFY_ORDER=0): storage order.
    uint32_t lbase = 0;    // byte offset of this lane's copy in pk
    bool lminus = false;   // walks its copy backwards
    if constexpr (RESIDENT) {
        static_assert(!RESIDENT || GW == 1, "the resident variants take one group per wave");
        if (a.xslot != nullptr) {
            const uint32_t g = g0 < a.G ? g0 : a.G - 1;
            const double delta = cw[0] - r_basef[0];
            const uint32_t mode = a.gmode[g];
            const bool near = !live[0] || !(__builtin_fabs(delta) >= a.gthr[g]) || (delta > 0.0 ? (mode & 1u) != 0u : (mode & 2u) != 0u);
            lminus = !near && delta < 0.0;
            lbase = near ? 0u : (uint32_t)sizeof(pk[0]);
        }
    }
    __syncthreads();
    uint32_t qn = a.qlen[q];
    uint32_t q_end = pos + first_lo + qn;  // one past the current query's last position
    bool fresh = true;  // the current query's lists are still empty (RESIDENT: filled by a sorting network)
    uint32_t nchain = 0;  // documents that made the wave run its insertion chain (reported per group: the host weighs the visiting-order upkeep against it)
    // RESIDENT: the run's walk tiles, from the one that holds its first document (a view's run may start inside one)
    uint32_t wti = 0, pb = pos, lo_first = first_lo;
    if constexpr (RESIDENT) {
        wti = a.run_wt0[r];
        pb = a.wt_start[wti];
        lo_first = pos + first_lo - pb;
    }
    bool first_tile = true;

    while (pb < run_end) {
        uint32_t pb_next = pb + (uint32_t)WAVE;
        if constexpr (RESIDENT) pb_next = a.wt_start[++wti];
        // documents of this step: the tile's, up to the run's end (behind a run's last tile comes padding, or -- a view --
        // documents that are not the run's)
        const uint32_t nvalid = (run_end < pb_next ? run_end : pb_next) - pb;
        const uint32_t lo_tile = first_tile ? lo_first : 0u;  // positions below it belong to no query of the run
        // ---------------- phase S: lane = document ----------------
        const float4* __restrict__ tile = RESIDENT ? nullptr : a.xb + (size_t)(pb >> 6) * dq * 64 + lane;
        float xf_res[RESIDENT ? DPL : GW];  // RESIDENT: the tile's x_f, loaded once
        double A[RESIDENT ? DPL : GW];
        uint32_t mycls[DPL], i0[DPL], i1[DPL];  // gain class | duplicate group; RESIDENT: where the document's word goes in the R-ordered / x_f-ordered copy
        if constexpr (RESIDENT) {
            constexpr int gi = 0;
            double t_inv, t_basef, tu_inv, tu_basef, tu_cand;
            {
                {
                    // One wave, one group: the group's six parameters come from the scalar cache once per tile instead of
                    // living in scalar registers across the document loop (where they were spilled to vector lanes and read
                    // back with a v_readlane each -- half of the tile step's vector instructions).
                    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                    typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
                    u32x4 p4;
                    u32x8 p8;
                    asm volatile("s_load_dwordx4 %0, %2, 0x0\n\ts_load_dwordx8 %1, %2, 0x10\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&s"(p4), "=&s"(p8) : "s"(par_g));  // (early-clobber: a destination that overlaps the address would be
                                                                          // overwritten by the first load while the second still waits to issue --
                                                                          // seen as a memory fault of the K = 10, XS = 2 variant at the 30K shape)
                    t_inv = __longlong_as_double((long long)(((uint64_t)p4.y << 32) | p4.x));
                    t_basef = __longlong_as_double((long long)(((uint64_t)p4.w << 32) | p4.z));
                    tu_inv = __longlong_as_double((long long)(((uint64_t)p8.w << 32) | p8.z));
                    tu_basef = __longlong_as_double((long long)(((uint64_t)p8.s5 << 32) | p8.s4));
                    tu_cand = __longlong_as_double((long long)(((uint64_t)p8.s7 << 32) | p8.s6));
                }
            }
            const uint32_t rslot_row = (uint32_t)a.rs_slot[g0 < a.G ? g0 : a.G - 1] >> 1;
#pragma unroll
            for (uint32_t h = 0; h < DPL; h++) {
                const uint32_t idx = lane + 64u * h;
                const bool mine = idx >= lo_tile && idx < nvalid;  // a document of the run
                const uint32_t p = pb + (idx < nvalid ? idx : 0u);  // (lanes beyond the tile re-read its first position: nothing of theirs is kept)
                double R = rcur[gi][p];
                if (r_upd[gi]) {  // the previous tick accepted a candidate for this restart
                    const double xu = (double)a.xcol[(size_t)u_f[gi] * a.np + p];
                    R = __builtin_fma(xu, tu_cand, __builtin_fma(-xu, tu_basef, R * tu_inv));
                    if (mine) roth[gi][p] = R;
                }
                // (from the column-major copy: in the tiles a column is one float in four of a 1 KB row, and the memory system
                // moves 16 bytes per document for the 4 that are used)
                xf_res[h] = a.xcol[(size_t)f[gi] * a.np + p];
                A[h] = __builtin_fma(-(double)xf_res[h], t_basef, R * t_inv);
                mycls[h] = a.gkey[p];
                i0[h] = i1[h] = idx;
                if (a.xslot != nullptr) {
                    i0[h] = a.rslot[(size_t)rslot_row * a.np + p];
                    i1[h] = a.xslot[(size_t)f[gi] * a.np + p];
                }
            }
        } else {
#pragma unroll
        for (int gi = 0; gi < GW; gi++) A[gi] = 0.0;
        for (uint32_t j4 = 0; j4 < dq; j4 += 8) {
            float4 xa[8];
#pragma unroll
            for (int u = 0; u < 8; u++) xa[u] = tile[(size_t)(j4 + u < dq ? j4 + u : dq - 1) * 64];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (j4 + u < dq) {
                    const double x0 = (double)xa[u].x, x1 = (double)xa[u].y, x2 = (double)xa[u].z, x3 = (double)xa[u].w;
#pragma unroll
                    for (int gi = 0; gi < GW; gi++) {
                        const double* wp = wl + gi * dp + (j4 + u) * 4;
                        A[gi] = __builtin_fma(x0, wp[0], A[gi]);
                        A[gi] = __builtin_fma(x1, wp[1], A[gi]);
                        A[gi] = __builtin_fma(x2, wp[2], A[gi]);
                        A[gi] = __builtin_fma(x3, wp[3], A[gi]);
                    }
                }
            }
        }
        }
        if constexpr (!RESIDENT) mycls[0] = a.gkey[pb + lane];
        __syncthreads();  // the previous tile's words have been consumed (one wave: cheap)
        if constexpr (RESIDENT) {
#pragma unroll
            for (uint32_t h = 0; h < DPL; h++) {
                const uint32_t idx = lane + 64u * h;
                // keys stay finite (the host refuses candidates whose products could overflow), so no NaN can slip
                // past a comparison below; a sum that is not comfortably finite sends the pair to the exact kernel
                // (only the run's own documents count: a view's tile may hold positions whose sums nobody keeps)
                redo[0] |= (idx >= lo_tile && idx < nvalid) && !(__builtin_fabs(A[h]) < 1e300);
                const uint64_t Ab = (uint64_t)__double_as_longlong(A[h]);
                const uint64_t Xb = (uint64_t)__double_as_longlong((double)xf_res[h]) | mycls[h];
                const uint4 word = make_uint4((uint32_t)Ab, (uint32_t)(Ab >> 32), (uint32_t)Xb, (uint32_t)(Xb >> 32));
                // (slots are positions inside the document's own segment of the tile -- a permutation of it, see
                // kernels_order.inc -- so the documents of the tile fill exactly the entries [0, nvalid) of both copies)
                if (idx < nvalid) {
                    pk[0][i0[h] & (VT - 1u)] = word;
                    pk[1][i1[h] & (VT - 1u)] = word;
                }
            }
        } else {
#pragma unroll
        for (int gi = 0; gi < GW; gi++) {
            const float xf = ((const float*)(tile + (size_t)(f[gi] >> 2) * 64))[f[gi] & 3];
            redo[gi] |= !(__builtin_fabs(A[gi]) < 1e300);
            const uint64_t Ab = (uint64_t)__double_as_longlong(A[gi]);
            const uint64_t Xb = (uint64_t)__double_as_longlong((double)xf) | mycls[0];
            pk[gi][lane] = make_uint4((uint32_t)Ab, (uint32_t)(Ab >> 32), (uint32_t)Xb, (uint32_t)(Xb >> 32));
        }
        }
        __syncthreads();
        // ---------------- phase K: lane = candidate ----------------
        uint32_t lo = lo_tile;
        while (lo < nvalid) {
            const uint32_t seg_hi = (q_end - pb) < nvalid ? (q_end - pb) : nvalid;
            if constexpr (RESIDENT) {
                // four documents per trip, read at constant offsets from the lane's own address: lanes of the backward
                // class start at the segment's end and step down (inside a trip they still go up -- any order is valid);
                // the segment's last n % 4 documents (for the backward class: its first) are one more, shorter trip
                const char* const pkb = reinterpret_cast<const char*>(&pk[0][0]) + lbase;
                // (only the lanes that carry a candidate execute the walk: 13 of 64 lanes idle at the reference's 51 candidates,
                // and a masked lane's datapath and registers stay still -- the socket runs this kernel at its power cap)
                if (VERIFY_LIVE_ONLY(live[0])) {
                uint32_t flo = lo, bhi = seg_hi;  // what is left of the segment: forward lanes [flo, seg_hi), backward lanes [lo, bhi)
                if (fresh && seg_hi - lo >= (uint32_t)KS && !(LS_DEBUG(a) & 1)) {
                    // the first KS documents of this lane's walk (backward lanes: the segment's last KS), four words per trip
                    uint32_t fa = (lminus ? seg_hi - 4u : lo) << 4;
                    const uint32_t fstep = lminus ? 0xFFFFFFC0u : 64u;
                    double fk[KS];
#pragma unroll
                    for (int i = 0; i + 4 <= KS; i += 4) {
                        const uint4 w0 = *reinterpret_cast<const uint4*>(pkb + fa), w1 = *reinterpret_cast<const uint4*>(pkb + fa + 16),
                                    w2 = *reinterpret_cast<const uint4*>(pkb + fa + 32), w3 = *reinterpret_cast<const uint4*>(pkb + fa + 48);
                        VERIFY_KEY(w0, fk[i])
                        VERIFY_KEY(w1, fk[i + 1])
                        VERIFY_KEY(w2, fk[i + 2])
                        VERIFY_KEY(w3, fk[i + 3])
                        fa += fstep;
                    }
                    if constexpr ((KS & 3) != 0) {
                        // the last KS % 4 of them: the next words going up for forward lanes, the words just below the trips above
                        // for backward lanes (whose next four-word trip would start 4 - KS % 4 words lower)
                        const uint32_t ta = lminus ? fa + (uint32_t)((4 - (KS & 3)) << 4) : fa;
                        const uint4 w0 = *reinterpret_cast<const uint4*>(pkb + ta);
                        VERIFY_KEY(w0, fk[KS & ~3])
                        if constexpr ((KS & 3) > 1) {
                            const uint4 w1 = *reinterpret_cast<const uint4*>(pkb + ta + 16);
                            VERIFY_KEY(w1, fk[(KS & ~3) + 1])
                        }
                        if constexpr ((KS & 3) > 2) {
                            const uint4 w2 = *reinterpret_cast<const uint4*>(pkb + ta + 32);
                            VERIFY_KEY(w2, fk[(KS & ~3) + 2])
                        }
                    }
                    verify_fill_sort<KS>(fk);
#pragma unroll
                    for (int m = 0; m < KS; m++) slot[0][m] = live[0] ? fk[m] : __builtin_huge_val();  // idle lanes admit nothing
                    flo = lo + (uint32_t)KS;
                    bhi = seg_hi - (uint32_t)KS;
                }
                const uint32_t n = (LS_DEBUG(a) & 1) ? 0u : seg_hi - flo, J = n >> 2, rem = n & 3u;  // (debug 1: phase S alone, timing only)
                uint32_t addr = (lminus ? bhi - 4u : flo) << 4;
                const uint32_t step = lminus ? 0xFFFFFFC0u : 64u;
                for (uint32_t j = 0; j < J; j++) {
                    const uint4 w0 = *reinterpret_cast<const uint4*>(pkb + addr), w1 = *reinterpret_cast<const uint4*>(pkb + addr + 16),
                                w2 = *reinterpret_cast<const uint4*>(pkb + addr + 32), w3 = *reinterpret_cast<const uint4*>(pkb + addr + 48);
                    VERIFY_VISIT(0, w0)
                    VERIFY_VISIT(0, w1)
                    VERIFY_VISIT(0, w2)
                    VERIFY_VISIT(0, w3)
                    addr += step;
                }
                if (rem != 0u) {
                    const uint32_t ta = (lminus ? lo : flo + (J << 2)) << 4;
                    const uint4 w0 = *reinterpret_cast<const uint4*>(pkb + ta), w1 = *reinterpret_cast<const uint4*>(pkb + ta + 16),
                                w2 = *reinterpret_cast<const uint4*>(pkb + ta + 32);  // (spare entries behind each copy)
                    VERIFY_VISIT(0, w0)
                    if (rem > 1u) VERIFY_VISIT(0, w1)
                    if (rem > 2u) VERIFY_VISIT(0, w2)
                }
                }
                fresh = false;
            } else {
#pragma unroll
            for (int gi = 0; gi < GW; gi++) {
                // four documents per trip: their words are read with constant LDS offsets, then handled in order
                for (uint32_t L = (LS_DEBUG(a) & 1) ? seg_hi : lo; L < seg_hi; L += 4) {  // (debug 1: phase S alone, timing only)
                    const uint4 w0 = pk[gi][L], w1 = pk[gi][L + 1], w2 = pk[gi][L + 2], w3 = pk[gi][L + 3];  // (3 spare entries)
                    VERIFY_VISIT(gi, w0)
                    if (L + 1 < seg_hi) VERIFY_VISIT(gi, w1)
                    if (L + 2 < seg_hi) VERIFY_VISIT(gi, w2)
                    if (L + 3 < seg_hi) VERIFY_VISIT(gi, w3)
                }
            }
            }
            if (q_end - pb > nvalid) break;  // the query continues in the next tile (q_end never lies behind the run's end)
            // ---- the current query is complete: NDCG@k (src/evaluators.rs:255-272,350-380) ----
            const double norm = a.norms[q];
            double rnorm = 0.0;  // (its reciprocal, or NaN where the quotient below must be a division)
            if constexpr (FAST_END) rnorm = a.rnorms[q];
            const double gam = a.gamma;  // (the relative part of a key's error bound: uniform)
            const uint32_t Ld = (uint32_t)a.depth < qn ? (uint32_t)a.depth : qn;
#pragma unroll
            for (int gi = 0; gi < GW; gi++) {
                if (live[gi]) {
                    double dcg = 0.0;
                    bool ok = true;
                    if constexpr (DUP) {
                        // Duplicate groups with mixed gains exist.  Documents of a query with bit-identical feature rows have
                        // bit-identical sums under every weight vector (the resident sums are seeded and updated by the same
                        // arithmetic on the same numbers), so their keys differ ONLY in the low bits, class | duplicate group:
                        // sorted, they come larger class id first = lower gain first -- the reference's tie-break
                        // (evaluators.rs:34-49: score, then gain ascending) -- so a pair of ONE group is in the reference's order
                        // as it stands.  What must still hold is that nothing else is tied with them: a maximal chain of close
                        // pairs -- a cluster -- is harmless iff all its documents carry one gain class (any order gives the same
                        // terms) or all its pairs are pairs of one duplicate group (the order is known); a mixture is not (a
                        // third document tied with the group could belong above or below all of it).  A cluster that reaches the
                        // cut must end, with a far pair, within the keys kept.
                        const uint32_t cmask = a.cls_only_mask, dmask = cls_mask & ~a.cls_only_mask;
                        bool allSame = true, allDup = true;  // the current cluster so far (reset behind a far pair)
#pragma unroll
                        for (int i = 0; i < K; i++) {
                            if ((uint32_t)i < Ld) {
                                const double hi = slot[gi][i], nx = slot[gi][i + 1];
                                // (the low bits as they were inserted: inverted in a negative key, see VERIFY_BITS_SRC)
                                const uint64_t hraw = (uint64_t)__double_as_longlong(hi), nraw = (uint64_t)__double_as_longlong(nx);
                                const uint64_t hb = hraw ^ (uint64_t)(verify_key_sign((uint32_t)(hraw >> 32)) & cls_mask);
                                const uint64_t nb = nraw ^ (uint64_t)(verify_key_sign((uint32_t)(nraw >> 32)) & cls_mask);
                                const uint32_t cls = (uint32_t)hb & cmask;
                                const double term = dtab[(uint32_t)i * ts + cls];
                                dcg = dcg + term;
                                ok &= (hi < __builtin_huge_val());  // false for +inf (and NaN)
                                if ((uint32_t)(i + 1) < qn) {  // a next document exists: slot i+1 holds its key
                                    const bool real = nx > NEG_INF;
                                    const bool far = verify_far(hi, nx, my_eps2[gi], gam) & real;
                                    const bool same = (((uint32_t)nb & cmask) == cls) & real;
                                    const bool dupp = real & (((hb ^ nb) & ~(uint64_t)cmask) == 0ull) & (((uint32_t)hb & dmask) != 0u);
                                    allSame = far | (allSame & same);
                                    allDup = far | (allDup & dupp);
                                    if ((uint32_t)(i + 1) < Ld) {
                                        ok &= allSame | allDup;  // both inside the cut (after a far pair both are true again)
                                    } else if constexpr (XS == 1) {
                                        ok &= far;
                                    } else {
                                        bool okc = far, cs = allSame, cd = allDup;
#pragma unroll
                                        for (int t = 1; t < XS; t++) {
                                            const double ka = slot[gi][i + t], kb = slot[gi][i + t + 1];
                                            const uint64_t kar = (uint64_t)__double_as_longlong(ka), kbr = (uint64_t)__double_as_longlong(kb);
                                            const uint64_t kab = kar ^ (uint64_t)(verify_key_sign((uint32_t)(kar >> 32)) & cls_mask);
                                            const uint64_t kbb = kbr ^ (uint64_t)(verify_key_sign((uint32_t)(kbr >> 32)) & cls_mask);
                                            const bool real_t = kb > NEG_INF;
                                            const bool far_t = ((uint32_t)(i + t + 1) >= qn) | (verify_far(ka, kb, my_eps2[gi], gam) & real_t);
                                            okc |= (cs | cd) & far_t;
                                            cs &= (((uint32_t)kbb & cmask) == cls) & real_t;
                                            cd &= real_t & (((kab ^ kbb) & ~(uint64_t)cmask) == 0ull) & (((uint32_t)kab & dmask) != 0u);
                                        }
                                        ok &= okc;
                                    }
                                }
                            }
                        }
                    } else {
                        // (no duplicate groups with mixed gains in this dataset: the plain walk -- close pairs must share a class)
                        const uint32_t cmask_plain = a.cls_only_mask;
                        if constexpr (XS == 1) {
                            // Straight-line for every query length: what depends on the length (Ld, qn) is uniform and only
                            // masks the lanes' decisions.  Rank i counts while i < Ld (past that its term comes from the zero
                            // row: adding +0.0 leaves the sum as it is -- it starts at +0.0 and is never -0.0); the pair
                            // (i, i + 1) must be far apart, or inside the cut of one class, if a document i + 1 exists.  The
                            // list is sorted, so the finiteness test of its largest key covers all of them.
                            //
                            // The pair test, cheap first.  In almost every wave every tested pair lies far apart, and then
                            // neither the exact bound nor the classes decide anything.  So each lane forms ONE bound for the
                            // whole query, tau >= verify_far's right-hand side for every pair its walk tests (verify_end.hpp:
                            // verify_gap_bound, from the larger magnitude of the first and the last key counted -- the list is
                            // sorted), and a rank costs the difference and one compare.  Only where some lane's pair is not
                            // beyond tau does the wave execute, for that rank alone, the test as it always stood -- verify_far,
                            // the class compare, the cut rule -- so what is decided is what was decided before, bit for bit:
                            // `diff > tau` implies `far`, and with `far` the rank leaves ok as it is.
                            ok = slot[gi][0] < __builtin_huge_val();
                            if constexpr (FAST_END) {
                                // the pairs tested: (i, i + 1) with i < Ld and i + 1 < qn, i.e. i < npair; the last key one of them
                                // reads is slot npair -- K for every query longer than a full-depth cut, and never a -inf of a
                                // short query's padding
                                const uint32_t npair = Ld < qn - 1u ? Ld : qn - 1u;  // (uniform)
                                double k_last = slot[gi][K];
                                if (npair < (uint32_t)K) {
#pragma unroll
                                    for (int m = 0; m < K; m++)
                                        if (npair == (uint32_t)m) k_last = slot[gi][m];
                                }
                                const double tau = verify_gap_bound(slot[gi][0], k_last, gam, my_eps2[gi]);
#pragma unroll
                                for (int i = 0; i < K; i++) {
                                    const bool counts = (uint32_t)i < Ld;
                                    const uint32_t lo_i = (uint32_t)__double_as_longlong(slot[gi][i]);
                                    const uint32_t roff = (counts ? (uint32_t)i : (uint32_t)K) * ts;  // (uniform)
                                    const double term = dtab[roff + (lo_i & cmask_plain)];
                                    const bool need = (uint32_t)i < npair;  // (uniform: ranks past a short query's end test nothing)
                                    const bool cheap_far = (slot[gi][i] - slot[gi][i + 1]) > tau;
                                    if (__builtin_expect(__ballot(need & !cheap_far) != 0ull, 0)) {
                                        const uint32_t lo_n = (uint32_t)__double_as_longlong(slot[gi][i + 1]);
                                        const bool incut = (uint32_t)(i + 1) < Ld;
                                        const bool far = verify_far(slot[gi][i], slot[gi][i + 1], my_eps2[gi], gam);
                                        const bool same = ((lo_i ^ lo_n) & cmask_plain) == 0u;
                                        ok &= far | (incut & same);
                                    }
                                    dcg = dcg + term;
                                    VERIFY_RANK_BARRIER
                                }
                            } else {
                                // (K = 5 and K = 20 keep every rank's exact test, see FAST_END; the ranks of K = 20 are not serialised
                                // either -- that costs more vector registers than the kernel has)
#pragma unroll
                                for (int i = 0; i < K; i++) {
                                    const bool counts = (uint32_t)i < Ld;
                                    const uint32_t lo_i = (uint32_t)__double_as_longlong(slot[gi][i]);
                                    const uint32_t lo_n = (uint32_t)__double_as_longlong(slot[gi][i + 1]);
                                    const uint32_t roff = (counts ? (uint32_t)i : (uint32_t)K) * ts;  // (uniform)
                                    const double term = dtab[roff + (lo_i & cmask_plain)];
                                    const bool need = counts && (uint32_t)(i + 1) < qn;
                                    const bool incut = (uint32_t)(i + 1) < Ld;
                                    const bool far = verify_far(slot[gi][i], slot[gi][i + 1], my_eps2[gi], gam);
                                    const bool same = ((lo_i ^ lo_n) & cmask_plain) == 0u;
                                    ok &= !need | far | (incut & same);
                                    dcg = dcg + term;
                                    if constexpr (K <= 10) { VERIFY_RANK_BARRIER }
                                }
                            }
                        } else {
    #pragma unroll
                        for (int i = 0; i < K; i++) {
                            if ((uint32_t)i < Ld) {
                                const double hi = slot[gi][i], nx = slot[gi][i + 1];
                                const uint32_t cls = (uint32_t)__double_as_longlong(hi) & cmask_plain;
                                double term = dtab[(uint32_t)i * ts + cls];
                                dcg = dcg + term;
                                ok &= (hi < __builtin_huge_val());  // false for +inf (and NaN)
                                if ((uint32_t)(i + 1) < qn) {  // a next document exists: slot i+1 holds its key
                                    const bool far = verify_far(hi, nx, my_eps2[gi], gam) & (nx > NEG_INF);
                                    const bool same = (((uint32_t)__double_as_longlong(nx) & cmask_plain) == cls) & (nx > NEG_INF);
                                    if ((uint32_t)(i + 1) < Ld) {
                                        ok &= far | same;  // both inside the cut: their order matters only across classes
                                    } else {
                                        // the cut: a tied cluster of one class may straddle it if it ends within the keys kept
                                        bool okc = far, chain = same;
    #pragma unroll
                                        for (int t = 1; t < XS; t++) {
                                            const double ka = slot[gi][i + t], kb = slot[gi][i + t + 1];
                                            const bool far_t = ((uint32_t)(i + t + 1) >= qn) | (verify_far(ka, kb, my_eps2[gi], gam) & (kb > NEG_INF));
                                            okc |= chain & far_t;
                                            chain &= (((uint32_t)__double_as_longlong(kb) & cmask_plain) == cls) & (kb > NEG_INF);
                                        }
                                        ok &= okc;
                                    }
                                }
                            }
                        }
                        }
                    }
                    double val = 0.0;
                    if (norm == norm) {
                        if (ok && dcg > norm) atomicOr(a.flags, FLAG_ACTUAL_GT_IDEAL);
                        // dcg / norm without the division where the host proved it (rnorm = fl(1 / norm); NaN = divide):
                        // five FMAs give the correctly rounded quotient, verify_end.hpp states the argument and its ranges
                        if constexpr (FAST_END) val = (rnorm == rnorm) ? verify_quotient(dcg, norm, rnorm) : dcg / norm;  // (uniform)
                        else val = dcg / norm;
                    }
                    a.M[(size_t)q * a.ldm + (size_t)(g0 + gi) * 64 + lane] = val;
                    qbad[gi] = !ok && !(LS_DEBUG(a) & 1);  // (debug 1: the walk's verdict is meaningless without phase K -- nothing is listed)
                } else {
                    qbad[gi] = false;
                }
            }
            // what the exact kernel has to recompute: the (query, group) pair with a mask of its 16-candidate slices that hold
            // an undecided candidate (redo[]: a non-finite sum earlier in this run -- every slice)
#pragma unroll
            for (int gi = 0; gi < GW; gi++) {
                const uint64_t bad = __ballot(qbad[gi]) | (__ballot(redo[gi]) != 0ull ? ~0ull : 0ull);
                if (g0 + gi < a.G && bad != 0ull && lane == 0) {
                    const uint32_t sm = ((bad & 0xFFFFull) ? 1u : 0u) | ((bad & 0xFFFF0000ull) ? 2u : 0u) | ((bad & 0xFFFF00000000ull) ? 4u : 0u) |
                                        ((bad >> 48) ? 8u : 0u);
                    uint32_t* const cnt = reinterpret_cast<uint32_t*>(a.redo_count);  // [0] pairs listed, [4 + g] pairs of group g
                    a.redo_list[atomicAdd(cnt, 1u)] = (q * a.G + g0 + gi) * 16u + sm;
                    atomicAdd(cnt + 4 + g0 + gi, 1u);
                }
            }
            lo = seg_hi;
            q++;
            if (q >= q1) break;
#pragma unroll
            for (int gi = 0; gi < GW; gi++)
#pragma unroll
                for (int m = 0; m < KS; m++) slot[gi][m] = live[gi] ? NEG_INF : __builtin_huge_val();
            qn = a.qlen[q];
            q_end += qn;
            fresh = true;
        }
        pb = pb_next;
        first_tile = false;
    }
    if (a.chain_count != nullptr && lane == 0 && nchain != 0u && g0 < a.G) atomicAdd(a.chain_count + g0, nchain);
}
#undef VERIFY_VISIT

// Applies pending resident-sum updates outside the verify kernel (ticks that go straight to the exact
// kernel): same arithmetic as the RESIDENT phase S.
__global__ void resident_update_kernel(LSArgs a) {
    const uint32_t g = a.g_base + blockIdx.y;
    const double* par = a.rs_par + (size_t)g * 6;
    if (par[2] == 0.0) return;
    const uint32_t p = posmap_position(a.posmap);
    if (p == IDX_INVALID) return;
    const int32_t sl = a.rs_slot[g];
    const uint32_t uf = a.rs_updf[g];
    const double xu = (double)a.xcol[(size_t)uf * a.np + p];  // (resident sums exist only next to the column-major copy)
    const double R = a.res_cur[(size_t)sl * a.np + p];
    a.res_cur[(size_t)(sl ^ 1) * a.np + p] = __builtin_fma(xu, par[5], __builtin_fma(-xu, par[4], R * par[3]));
}

// FR_VERIFY_AUDIT: bitwise comparison of two result matrices (published values vs the exact kernel's).
__global__ void audit_compare_kernel(const double* a, const double* b, size_t n, unsigned long long* cnt) {
    unsigned long long bad = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        bad += __double_as_longlong(a[i]) != __double_as_longlong(b[i]) ? 1ull : 0ull;
    if (bad) atomicAdd(cnt, bad);
}
