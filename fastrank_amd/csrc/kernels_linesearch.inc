// Part of device.hip (single translation unit; see that file's header).  The fused NDCG@k coordinate-ascent line-search kernel (the hot path).
struct LSArgs {
    const float4* xb;         // feature tiles
    const uint32_t* gcls;     // [np] gain class of each document
    const double* dcgtab;     // [ncls][LS_KT]: (2^gain - 1) / log2(i + 2), divided on the host
    const uint32_t* qstart;   // [nq] padded start position
    const uint32_t* qlen;     // [nq]
    const uint32_t* run_q0;   // [nruns] first query of the run
    const uint32_t* run_q1;   // [nruns] one past its last query
    const uint32_t* run_pos;  // [nruns] position of the tile the run starts in (multiple of 64)
    const uint32_t* run_lo;   // [nruns] lanes of that tile that precede the run (0 unless the dataset is a view of another's tiles)
    const uint32_t* run_docs; // [nruns] documents in the run
    const uint32_t* run_order;// [nruns] longest-first schedule
    const uint32_t* wt_start; // [walk tiles + 1] RESIDENT verify kernel: first position of every walk tile (kernels_order.inc)
    const uint32_t* run_wt0;  // [nruns] ... and the walk tile that holds the run's first document
    const double* norms;
    const double* rnorms;     // [nq] verify kernel: fl(1 / norms[q]) where verify_quotient (verify_end.hpp) stands for the division, NaN elsewhere
    const double* disc;
    const uint32_t* gfeat;    // [G]
    const double* gw;         // [G][4*dq] zero padded
    const double* gcand;      // [G][64]
    const uint32_t* gncand;   // [G]
    double* M;                // [nq][ldm]
    int* flags;
    unsigned long long* dbg_counters;  // [4] rows, batches, insertion rows, documents (debug bit 16)
    // bound-and-verify (kernels_verify.inc): eps2[g][c] = twice the bound on |approximate - exact score| of any
    // document for that candidate; (query, group) pairs it could not verify are appended to redo_list as q * G + g
    const double* eps2;       // [G][64]  (the NDCG@k verify kernel: the ABSOLUTE part of a pair's bound; its relative part is gamma)
    double gamma;             // a key's error bound is eps2 / 2 + gamma * |key| (kernels_verify.inc, verify_far)
    // The redo list: entry = (q * G + g) * 16 + mask, one per (query, group) pair the verify kernel could not decide; bit s
    // of the mask = the pair's 16-candidate slice s holds an undecided candidate.  The exact kernel gives every entry four
    // blocks, one per slice, and a block whose bit is clear returns at once: a tie that only the `dir = 0` candidate sees
    // (src/coordinate_ascent.rs:152-155) costs one block of 16 accumulators per document, not four.
    unsigned long long* redo_count;  // low word: pairs listed; high word: slices the exact kernel recomputed; behind them, from
                              // byte 16 on, 32-bit counts of the pairs listed per group (the host routes a restart whose line
                              // searches keep failing to the exact kernel): one 16-byte slot + G words of the tick block
    uint32_t* redo_list;      // [nq * G]
    uint32_t* chain_count;    // [G] verify kernel (or nullptr): documents per group that made a wave run its insertion chain, summed over the runs
    const uint32_t* work_list;  // exact kernel: if non-null, blocks 4 b .. 4 b + 3 recompute the slices of entry work_list[b] (CT <= 16)
    const uint32_t* work_count; // with work_list: if non-null, blocks of entries at or past *work_count have nothing to do (the
                                // grid is a fixed size so that the host need not read the count between the two launches)
    uint32_t* slice_count;      // with work_list: counts the blocks that had work
    uint32_t g_base;            // exact kernel without work_list, resident_update_kernel: the launch covers groups [g_base, g_base + G)
    uint32_t cls_mask;        // verify kernel: low mantissa bits that carry the document's gain class and duplicate group
    uint32_t cls_only_mask;   // ... of which the gain class
    const uint16_t* gkey;     // [np] class | duplicate group << class bits (verify kernel)
    // resident base sums (verify kernel, RESIDENT): per group, see LineGroup in device.hpp
    double* res_cur;          // [slots][2][np]: buffer (slot, half) holds R; updates are written to the other half
    const int32_t* rs_slot;   // [G] slot * 2 + current half
    const double* rs_par;     // [G][6]: norm, base_f, has_update, upd_norm, upd_base_f, upd_cand
    const float* xcol;        // [d][np] the tiles' columns, column-major; never nullptr where the RESIDENT kernels run (resident_reserve
                              // refuses a dataset without it, and the trainer then forms its sums from the tiles with the GW >= 1 variants)
    const uint32_t* rs_updf;  // [G] feature of the pending update
    // visiting order of the RESIDENT verify kernel (kernels_verify.inc): slot of every document inside its (query, tile)
    // segment by x_f descending (static, per feature) / by R descending (per resident slot); per group the |w_c - base_f|
    // below which a candidate walks the R-ordered copy, and bit 0 / 1 = candidates above / below it do so too
    const uint8_t* xslot;     // [d][np] (nullptr: storage order)
    const uint8_t* rslot;     // [slots][np]
    const double* gthr;       // [G]
    const uint32_t* gmode;    // [G]
    uint32_t np;
    PosMap posmap;            // resident_update_kernel: the positions to visit (a view: its own tiles only)
    uint32_t dq, d, nruns, G, ldm;
    uint32_t ncls;            // gain classes (rows of dcgtab)
    int depth;
#ifdef FR_PRICING
    int debug;  // pricing builds only (-DFR_PRICING, env FR_LS_DEBUG): 1 = skip phase K, 2 = no threshold filter, 16 = count rows
#endif
};
// The timing ablations of FR_LS_DEBUG return wrong numbers by design, so the field and every branch on it exist only in
// a pricing build; in the shipped library LS_DEBUG(a) is the constant 0 and the branches fold away.
#ifdef FR_PRICING
#define LS_DEBUG(A) ((A).debug)
#define LS_DEBUG_SET(A, V) ((A).debug = (V))
#else
#define LS_DEBUG(A) 0
#define LS_DEBUG_SET(A, V) ((void)(V))
#endif

constexpr int LS_ROWPAD = 65;  // LDS row stride in doubles: 130 dwords -> 16 lanes hit 16 distinct even banks
constexpr int LS_KT = 20;      // ranks covered by the per-gain-class DCG term table
#ifndef LS_WAVES_PER_SIMD
#define LS_WAVES_PER_SIMD 3
#endif

__device__ __forceinline__ uint64_t lane_range_mask(uint32_t lo, uint32_t hi) {
    const uint64_t up = (hi >= 64u) ? ~0ull : ((1ull << hi) - 1ull);
    return up & ~((1ull << lo) - 1ull);
}

// The fused line search.  One wave per (run of consecutive queries, line group); CT = candidate
// tile (accumulators per lane in phase S), K = top-K list length (>= depth), RB = documents per
// transpose batch.
//
// phase S (lane = document, one 64-document tile per step; tiles are full because a run packs
//   several queries): exact ordered f64 dot products for all CT candidates at once.  The prefix
//   sum over features < f is shared by every candidate and so are the products x_j*w_j (j > f):
//   a candidate costs one v_add_f64 per feature.  Features arrive four at a time (16-byte loads,
//   prefetched two groups ahead); weights come from LDS where two masked copies (w_j for j < f,
//   w_j for j > f, zero elsewhere) remove every per-feature branch: a masked product is +-0.0 and
//   adding it changes nothing, because a sum that starts at +0.0 can never be -0.0.
// filter: a document can only matter if it ties/beats the current K-th best score of at least one
//   candidate; thresholds are re-published after every transpose batch.
// phase K (lane = candidate): surviving documents of the current query are transposed through LDS
//   in batches of RB rows and inserted, in document order, into each candidate's sorted top-K
//   list (registers).  At a query boundary inside the tile the lists are turned into NDCG@k.
template <int K, int CT, int RB>
__global__ __launch_bounds__(WAVE, CT <= 16 ? 2 : LS_WAVES_PER_SIMD) void linesearch_ndcg_kernel(LSArgs a) {  // (narrow: registers for the load ring, see phase S)
    extern __shared__ __attribute__((aligned(16))) double wdyn[];  // wpre[4*dq], wsuf[4*dq]
    __shared__ double tr[RB * LS_ROWPAD];
    __shared__ double thr[WAVE];
    __shared__ double cwl[WAVE];  // this group's candidate weights for feature f
    __shared__ uint32_t rowcls[RB];
    const uint32_t lane = threadIdx.x;
    // XCD-aware block -> (run, group): blocks b, b+8, b+16.. run on one XCD (observed dispatch
    // b % 8), so all groups of a run share that XCD's L2 for the run's feature tiles.
    uint32_t g, q, q1, pos, run_end, first_lo = 0, cand0 = 0;
    if (a.work_list != nullptr) {
        // redo mode: one (query, group) pair the verify kernel could not decide.  The query is processed like a
        // run of its own, in stretches of 64 positions from its FIRST document (a lane reads its position's tile:
        // a stretch lies across two) -- 2 stretches for 120 documents where the tiles they lie in are 2.9.
        const uint32_t e = blockIdx.x >> 2, sl = blockIdx.x & 3u;
        if (a.work_count != nullptr && e >= *a.work_count) return;
        const uint32_t entry = a.work_list[e];
        if (((entry >> sl) & 1u) == 0u) return;
        cand0 = sl * 16u;  // (a slice is 16 candidates whatever CT <= 16 the launch was compiled for)
        const uint32_t item = entry >> 4;
        g = item % a.G;
        q = item / a.G;
        q1 = q + 1;
        const uint32_t qs = a.qstart[q];
        pos = qs;
        run_end = qs + a.qlen[q];
    } else {
        const uint32_t blk = blockIdx.x;
        const uint32_t xcd = blk & 7u, seq = blk >> 3;
        g = a.g_base + seq % a.G;
        const uint32_t ri = (seq / a.G) * 8u + xcd;
        if (ri >= a.nruns) return;
        const uint32_t r = a.run_order[ri];
        q = a.run_q0[r];
        q1 = a.run_q1[r];
        pos = a.run_pos[r];
        first_lo = a.run_lo[r];
        run_end = pos + a.run_docs[r];
    }
    const uint32_t f = a.gfeat[g];
    // (a slice of the candidates in sliced work-list mode: lane c stands for candidate cand0 + c)
    const uint32_t ncand_all = a.gncand[g];
    const uint32_t ncand = ncand_all > cand0 ? (ncand_all - cand0 < (uint32_t)CT ? ncand_all - cand0 : (uint32_t)CT) : 0u;
    if (ncand == 0u) return;
    if (a.work_list != nullptr && a.slice_count != nullptr && lane == 0) atomicAdd(a.slice_count, 1u);
    const uint32_t dq = a.dq, dp = a.dq * 4, d = a.d;
    const double* __restrict__ w = a.gw + (size_t)g * dp;
    const double NEG_INF = -__builtin_huge_val();
    double* wpre = wdyn;
    double* wsuf = wdyn + dp;
    for (uint32_t j = lane; j < dp; j += WAVE) {
        const double wv = j < d ? w[j] : 0.0;
        wpre[j] = j < f ? wv : 0.0;
        wsuf[j] = j > f ? wv : 0.0;
    }
    thr[lane] = NEG_INF;  // nothing is filtered until a candidate's list is full
    cwl[lane] = a.gcand[(size_t)g * 64 + (cand0 + lane < 64u ? cand0 + lane : 63u)];
    __syncthreads();

    double slot_s[K];
    uint32_t slot_c[K];  // gain class of the document in each slot
#pragma unroll
    for (int m = 0; m < K; m++) {
        slot_s[m] = NEG_INF;
        slot_c[m] = 0;
    }
    bool nan_seen = false;
    uint32_t dbg_rows = 0, dbg_batches = 0, dbg_ins = 0;
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint32_t qn = a.qlen[q];
    uint32_t q_end = pos + first_lo + qn;  // one past the current query's last position
    const uint32_t ngp = (f + 3) >> 2;   // tile groups that hold prefix features
    const uint32_t sq0 = (f + 1) >> 2;   // first tile group that holds a suffix feature
    const uint32_t fgrp = f >> 2, fsub = f & 3;

    // the narrow instantiations' load stream (see phase S): a stretch's feature groups in order, padded with repeats of its last
    // group to a multiple of LS_RING requests (slot u of the ring then always holds element u mod LS_RING of a stretch: static
    // register indices, no rotation -- a register move would wait for the load it moves); past the last stretch the stream
    // repeats that stretch (requests nobody reads)
    constexpr int LS_RING = 8;
    float4 xq[CT <= 16 ? LS_RING : 1];
    const uint32_t dq_ring = (dq + (uint32_t)LS_RING - 1u) / (uint32_t)LS_RING * (uint32_t)LS_RING;
    uint32_t ld_pb = pos, ld_e = 0;
    size_t ld_base = 0;
#define LS_RING_BASE()                                                                     \
    {                                                                                      \
        const uint32_t lp_ = ld_pb + lane < a.np ? ld_pb + lane : a.np - 1u;               \
        ld_base = (size_t)(lp_ >> 6) * dq * 64 + (lp_ & 63u);                              \
    }
#define LS_RING_LOAD(DST)                                                                  \
    {                                                                                      \
        DST = a.xb[ld_base + (size_t)(ld_e < dq ? ld_e : dq - 1u) * 64];                   \
        if (++ld_e == dq_ring) {                                                           \
            ld_e = 0;                                                                      \
            if (ld_pb + (uint32_t)WAVE < run_end) ld_pb += (uint32_t)WAVE;                 \
            LS_RING_BASE()                                                                 \
        }                                                                                  \
    }
    if constexpr (CT <= 16) {
        LS_RING_BASE()
#pragma unroll
        for (int u = 0; u < LS_RING; u++) LS_RING_LOAD(xq[u])
    }
    for (uint32_t pb = pos; pb < run_end; pb += WAVE) {
        // ---------------- phase S: lane = document ----------------
        double sc[CT];
        uint32_t mycls;
        if constexpr (CT <= 16) {
            // The narrow instantiations serve the redo launches (dispatch_exact): a few thousand one-wave blocks whose launch lasts
            // as long as its longest query -- 876 documents = 14 stretches one after the other, each a chain of memory round
            // trips (measured on hardties data: 200 us per launch with 340 waves resident on average, 63 % of their cycles
            // waiting).  So the feature groups of a stretch are ONE stream, prefix and suffix alike, with LS_RING of them in
            // flight, and the stream runs on into the next stretch while this one's documents are inserted.  The arithmetic is
            // the same sequence as below: a group's prefix products (masked weights), the candidates' start at the group of
            // feature f, the suffix products.  Measured (profiles/r06_exact_redo.txt): 214 -> 130 us per launch, a hardties
            // step 3.15 -> 3.07 ms (2.97 with no redo at all); a ring of 12: 127 us; the same ring rotated through register
            // moves: 206 us.
            mycls = a.gcls[pb + lane < a.np ? pb + lane : a.np - 1u];
            double P = 0.0;
            for (uint32_t j0 = 0; j0 < dq_ring; j0 += (uint32_t)LS_RING) {
#pragma unroll
                for (int u = 0; u < LS_RING; u++) {
                    const uint32_t j4 = j0 + (uint32_t)u;
                    const float4 cur = xq[u];
                    if (j4 < dq) {
                        if (j4 < ngp) {
                            const double* wp = wpre + j4 * 4;
                            double p0 = (double)cur.x * wp[0];
                            P = P + p0;
                            double p1 = (double)cur.y * wp[1];
                            P = P + p1;
                            double p2 = (double)cur.z * wp[2];
                            P = P + p2;
                            double p3 = (double)cur.w * wp[3];
                            P = P + p3;
                        }
                        if (j4 == fgrp) {
                            const double xf = (double)(fsub == 0 ? cur.x : (fsub == 1 ? cur.y : (fsub == 2 ? cur.z : cur.w)));
#pragma unroll
                            for (int c = 0; c < CT; c++) {
                                double prod = xf * cwl[c];
                                sc[c] = P + prod;
                            }
                        }
                        if (j4 >= sq0) {
                            const double* wp = wsuf + j4 * 4;
                            const float xs[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
                            for (int v = 0; v < 4; v++) {
                                double prod = (double)xs[v] * wp[v];
#pragma unroll
                                for (int c = 0; c < CT; c++) sc[c] = sc[c] + prod;
                            }
                        }
                    }
                    LS_RING_LOAD(xq[u])  // (the element LS_RING further on, into the slot just read)
                    __builtin_amdgcn_sched_barrier(0);  // (slot by slot: interleaved, their temporaries take the registers the ring needs)
                }
            }
        } else {
            const float4* __restrict__ tile = a.xb + (size_t)(pb >> 6) * dq * 64 + lane;
            mycls = a.gcls[pb + lane];
            double P = 0.0;  // shared prefix: features < f in order (dense_dataset.rs:71-74)
            if (ngp > 0) {
                float4 xa[4], xc[4];
    #pragma unroll
                for (int u = 0; u < 4; u++) xa[u] = tile[(size_t)((uint32_t)u < ngp ? (uint32_t)u : ngp - 1) * 64];
                for (uint32_t j4 = 0; j4 < ngp; j4 += 4) {
    #pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint32_t jn = j4 + 4 + u;
                        xc[u] = tile[(size_t)(jn < ngp ? jn : ngp - 1) * 64];
                    }
    #pragma unroll
                    for (int u = 0; u < 4; u++) {
                        if (j4 + u < ngp) {
                            const double* wp = wpre + (j4 + u) * 4;
                            double p0 = (double)xa[u].x * wp[0];
                            P = P + p0;
                            double p1 = (double)xa[u].y * wp[1];
                            P = P + p1;
                            double p2 = (double)xa[u].z * wp[2];
                            P = P + p2;
                            double p3 = (double)xa[u].w * wp[3];
                            P = P + p3;
                        }
                    }
    #pragma unroll
                    for (int u = 0; u < 4; u++) xa[u] = xc[u];
                }
            }
            const double xf = (double)((const float*)(tile + (size_t)fgrp * 64))[fsub];
            // two tile groups of the suffix are requested before the candidate initialisation
            float4 x0 = tile[(size_t)(sq0 < dq ? sq0 : dq - 1) * 64];
    #pragma unroll
            for (int c = 0; c < CT; c++) {
                double prod = xf * cwl[c];
                sc[c] = P + prod;
            }
            for (uint32_t j4 = sq0; j4 < dq; j4++) {
                const float4 x2 = tile[(size_t)(j4 + 1 < dq ? j4 + 1 : dq - 1) * 64];
                const double* wp = wsuf + j4 * 4;
                const float xs[4] = {x0.x, x0.y, x0.z, x0.w};
    #pragma unroll
                for (int u = 0; u < 4; u++) {
                    double prod = (double)xs[u] * wp[u];
    #pragma unroll
                    for (int c = 0; c < CT; c++) sc[c] = sc[c] + prod;
                }
                x0 = x2;
            }
        }
        // ---------------- filter + transpose + phase K: lane = candidate ----------------
        const uint32_t nvalid = (run_end - pb) < (uint32_t)WAVE ? (run_end - pb) : (uint32_t)WAVE;
        uint32_t lo = (pb == pos) ? first_lo : 0u;
        while (lo < nvalid) {
            const uint32_t seg_hi = (q_end - pb) < nvalid ? (q_end - pb) : nvalid;
            uint64_t remaining = lane_range_mask(lo, seg_hi);
            if (LS_DEBUG(a) & 1) remaining = 0ull;
            while (remaining != 0ull) {
                if (!(LS_DEBUG(a) & 2)) {
                    bool p = false;
#pragma unroll
                    for (int c = 0; c < CT; c++) p |= (sc[c] >= thr[c]) | (sc[c] != sc[c]);
                    remaining &= __ballot(p);
                    if (remaining == 0ull) break;
                }
                const bool mine = (remaining >> lane) & 1ull;
                const uint32_t myrank = __popcll(remaining & lt_mask);
                const bool in_batch = mine && myrank < (uint32_t)RB;
                if (in_batch) {
                    double* row = tr + myrank * LS_ROWPAD;
#pragma unroll
                    for (int c = 0; c < CT; c++) row[c] = sc[c];
                    rowcls[myrank] = mycls;
                }
                const uint64_t batch_mask = __ballot(in_batch);
                const uint32_t nb = __popcll(batch_mask);
                remaining &= ~batch_mask;
                dbg_rows += nb;
                dbg_batches++;
                __syncthreads();
                for (uint32_t rr = 0; rr < nb; rr++) {
                    const double e = lane < (uint32_t)CT ? tr[rr * LS_ROWPAD + lane] : NEG_INF;
                    const uint32_t ep = rowcls[rr];
                    nan_seen |= (e != e);
                    if (__ballot(e >= slot_s[K - 1]) != 0ull) {
                        dbg_ins++;
                        // ordered insertion: e goes above every slot it ties or beats (later document
                        // wins ties = reference tie-break in the reverse layout).  Empty slots hold
                        // -inf and therefore lose against every non-NaN score, including -inf itself.
                        bool beat[K];
#pragma unroll
                        for (int m = 0; m < K; m++) beat[m] = (e >= slot_s[m]);
#pragma unroll
                        for (int m = K - 1; m >= 1; m--) {
                            slot_s[m] = beat[m - 1] ? slot_s[m - 1] : (beat[m] ? e : slot_s[m]);
                            slot_c[m] = beat[m - 1] ? slot_c[m - 1] : (beat[m] ? ep : slot_c[m]);
                        }
                        slot_s[0] = beat[0] ? e : slot_s[0];
                        slot_c[0] = beat[0] ? ep : slot_c[0];
                    }
                }
                // publish each candidate's K-th best score; unused candidate lanes never admit a document
                thr[lane] = (lane < ncand) ? slot_s[K - 1] : __builtin_huge_val();
                __syncthreads();
            }
            if (q_end - pb > (uint32_t)WAVE) break;  // the query continues in the next tile
            // ---- the current query is complete: NDCG@k (src/evaluators.rs:255-272,350-380) ----
            if (lane < ncand) {
                const uint32_t L = (uint32_t)a.depth < qn ? (uint32_t)a.depth : qn;
                double dcg = 0.0;
#pragma unroll
                for (int i = 0; i < K; i++) {
                    if ((uint32_t)i < L) {
                        double term = a.dcgtab[(size_t)slot_c[i] * LS_KT + i];
                        dcg = dcg + term;
                    }
                }
                const double norm = a.norms[q];
                double val = 0.0;
                int fl = 0;
                if (norm == norm) {
                    if (dcg > norm) fl |= FLAG_ACTUAL_GT_IDEAL;
                    val = dcg / norm;
                }
                if (fl && !LS_DEBUG(a)) atomicOr(a.flags, fl);
                a.M[(size_t)q * a.ldm + (size_t)g * 64 + cand0 + lane] = val;
            }
            lo = seg_hi;
            q++;
            if (q >= q1) break;
#pragma unroll
            for (int m = 0; m < K; m++) {
                slot_s[m] = NEG_INF;
                slot_c[m] = 0;
            }
            qn = a.qlen[q];
            q_end += qn;
            __syncthreads();  // every lane has read thr[] for the finished query
            thr[lane] = NEG_INF;
            __syncthreads();
        }
    }
    if (nan_seen && !LS_DEBUG(a)) atomicOr(a.flags, FLAG_NAN_SCORE);
    if ((LS_DEBUG(a) & 16) && lane == 0) {
        atomicAdd(a.dbg_counters + 0, (unsigned long long)dbg_rows);
        atomicAdd(a.dbg_counters + 1, (unsigned long long)dbg_batches);
        atomicAdd(a.dbg_counters + 2, (unsigned long long)dbg_ins);
        atomicAdd(a.dbg_counters + 3, (unsigned long long)(run_end - pos));
    }
}
#undef LS_RING_LOAD
#undef LS_RING_BASE

