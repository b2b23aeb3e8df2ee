// Part of device.hip (single translation unit; see that file's header).  The ApproxNDCG objective (DESIGN.md section 11,
// "ApproxNDCG objective"): the gradient of the smooth NDCG of every query, two n^2 passes with one exp per unordered pair.
//
// Definition, for one query of n documents in STORED order (instance ids ascending: lm_pos lists their positions), all f64;
// G_i = gexp_i, N = the NDCG evaluator's norm of the query, alpha = the request's sigma:
//   sig(t)   = 1 / (1 + exp(-t))
//   q_ij     = sig(alpha (s_j - s_i)) for i < j;  q_ji = 1 - q_ij (rounded)
//   p_ij     = p_ji = q_ij (1 - q_ij), from the q of i < j
//   r_i      = 1 + sum_{j != i} q_ij                            (the soft rank: a tie counts one half)
//   A        = (1 / N) sum_i G_i / log2(1 + r_i)                (the objective; no kernel needs its value)
//   c_i      = -((G_i / N) / (((1 + r_i) LN2) (log2(1 + r_i))^2))                                  (dA / dr_i)
//   lambda_k = alpha sum_{i != k} (c_i - c_k) p_ik              (dA / ds_k, the ascent direction);  w_k = 0
// Both sums are ONE chain per document: from +0.0, the partners in ascending stored order, the document itself left out;
// r_i = 1.0 + that chain, lambda_k = alpha * that chain.  Every operation is rounded where it is written (-ffp-contract=off),
// t = alpha * (s_j - s_i), LN2 = 0x1.62e42fefa39efp-1.  A query of one document, or whose norm is NaN or not positive, gets
// lambda = w = 0.  Non-finite scores propagate as IEEE arithmetic gives: no index depends on a score.
//
// Work.  The pair matrix is cut into 64 x 64 tiles (I, J), I <= J, of which only the upper triangle is ever computed: one exp
// per unordered pair and pass.  A tile's terms are produced 64 wide into a padded LDS tile (64 rows of AX_LD = 65 doubles: a
// row walk and a column walk are both conflict-free), then summed: lane a of one wave adds row a's terms to document
// 64 I + a with b ascending, lane b of another wave adds column b's mirrored terms (1 - q, or the same p) to document 64 J + b
// with a ascending.  Tiles are visited with J ascending and, under it, I = 0 .. J: document i meets (0, I) .. (I - 1, I) as a
// column, the diagonal tile (I, I) (its column half up to i, then its row half), then (I, I + 1) .. as a row -- the
// definition's chain, partner by partner.  The diagonal tile is filled by the circulant (a, a + d mod 64), d = 1 .. 32, so
// that its 2016 pairs cost 32 exp steps, not 63.
//   n <= 64           lambda_grad_approx_wave_kernel: a wave per query, four queries per workgroup, each wave with a tile of
//                     its own.  The query is its diagonal tile; pass 2 turns the cached q into p in place, so the whole
//                     query costs one exp per unordered pair.
//   64 < n <= 256     lambda_grad_approx_kernel, a workgroup per query: scores, chains and c staged in LDS; the four waves fill
//                     a tile together (16 columns or 8 circulant steps each), waves 0 and 1 sum it.  Pass 2 computes q again
//                     (two exps per unordered pair in all): the q of a long query does not fit anywhere.
//   n > 256           the same statements with the query left in memory: the chains live in the output arrays (r, then c in
//                     wt; lambda's chain in lam), and the scores and c of a tile's two blocks are read again (L2 hits) into
//                     LDS before every tile, at the price of a third barrier per tile.
// Same operands, same operations, same order on every path: a query's bits do not depend on its path or its neighbours.
// No atomics, no scratch; the barriers of a workgroup do not depend on data.

constexpr int LM_OBJ_APPROX = 8;
static_assert(LM_OBJ_APPROX == LM_OBJECTIVE_APPROXNDCG, "the ApproxNDCG objective's id is the host's");
constexpr uint32_t AX_LD = 65;                 // doubles per tile row
constexpr uint32_t AX_TILE = 64 * AX_LD;       // doubles per tile
constexpr uint32_t AX_WAVES = 4;               // waves per workgroup: queries (wave kernel) or tile quarters (group kernel)
constexpr uint32_t AX_WAVE_MAX = 64;           // the longest query a wave takes
constexpr uint32_t AX_STAGE = 256;             // the longest query staged in LDS
constexpr double AX_LN2 = 0x1.62e42fefa39efp-1;
constexpr size_t AX_WAVE_LDS = (size_t)AX_WAVES * (AX_TILE + 128) * sizeof(double);  // per wave: tile, s[64], c[64]
constexpr size_t AX_GROUP_LDS = (size_t)(AX_TILE + 3 * AX_STAGE) * sizeof(double);  // tile, s, r / c, lambda's chain

// q_ij of i < j
__device__ __forceinline__ double ax_q(double si, double sj, double alpha) {
    const double d = sj - si;
    const double t = alpha * d;
    const double e = exp(-t);
    return 1.0 / (1.0 + e);
}

// c_i from the chain of pass 1
__device__ __forceinline__ double ax_c(double chain, double G, double norm) {
    const double r = 1.0 + chain;
    const double x = 1.0 + r;
    const double l = log2(x);
    const double g = G / norm;
    const double den = (x * AX_LN2) * (l * l);
    return -(g / den);
}

// W waves fill tile (I, J): q (pass 1) or p (P2) of every pair (64 I + a, 64 J + b) below n, at tile[a * AX_LD + b]; on the
// diagonal only a < b.  wv: this wave's index among the W.  S(i): the score of document i.
template <uint32_t W, bool P2, class SF>
__device__ __forceinline__ void ax_fill(double* tile, uint32_t I, uint32_t J, uint32_t n, uint32_t wv, uint32_t lane, double alpha, SF S) {
    if (I == J) {
        constexpr uint32_t steps = 32 / W;
        for (uint32_t k = 0; k < steps; k++) {
            const uint32_t d = wv * steps + k + 1, o = (lane + d) & 63u;
            const uint32_t a = min(lane, o), b = max(lane, o);
            if ((d == 32 && lane >= 32) || 64 * I + b >= n) continue;  // (the pair of d = 32 belongs to its lower lane)
            const double q = ax_q(S(64 * I + a), S(64 * I + b), alpha);
            tile[a * AX_LD + b] = P2 ? q * (1.0 - q) : q;
        }
    } else {
        constexpr uint32_t cols = 64 / W;
        const double si = S(64 * I + lane);  // (I < J: the whole row block lies below n)
        for (uint32_t k = 0; k < cols; k++) {
            const uint32_t b = wv * cols + k, j = 64 * J + b;
            if (j >= n) break;
            const double q = ax_q(si, S(j), alpha);
            tile[lane * AX_LD + b] = P2 ? q * (1.0 - q) : q;
        }
    }
}

// One wave, lane a = document 64 I + a, continues its chain over the diagonal tile: the partners of block I, ascending.
// ACC(i): the chain of document i (a reference); C(i): c_i (pass 2 only).
template <bool P2, class AF, class CF>
__device__ __forceinline__ void ax_sum_diag(const double* tile, uint32_t I, uint32_t n, uint32_t lane, AF ACC, CF C) {
    const uint32_t i = 64 * I + lane;
    if (i >= n) return;
    const uint32_t nb = min(64u, n - 64 * I);
    double acc = ACC(i);
    const double ci = P2 ? C(i) : 0.0;
    for (uint32_t b = 0; b < nb; b++) {
        if (b == lane) continue;
        const double v = tile[b < lane ? b * AX_LD + lane : lane * AX_LD + b];
        if constexpr (P2) acc = acc + (C(64 * I + b) - ci) * v;
        else acc = acc + (b < lane ? 1.0 - v : v);
    }
    ACC(i) = acc;
}

// ... over an off-diagonal tile as a row (lane a = document 64 I + a, partners 64 J + b ascending)
template <bool P2, class AF, class CF>
__device__ __forceinline__ void ax_sum_row(const double* tile, uint32_t I, uint32_t J, uint32_t n, uint32_t lane, AF ACC, CF C) {
    const uint32_t i = 64 * I + lane, nb = min(64u, n - 64 * J);
    double acc = ACC(i);
    const double ci = P2 ? C(i) : 0.0;
    for (uint32_t b = 0; b < nb; b++) {
        const double v = tile[lane * AX_LD + b];
        if constexpr (P2) acc = acc + (C(64 * J + b) - ci) * v;
        else acc = acc + v;
    }
    ACC(i) = acc;
}

// ... and as a column (lane b = document 64 J + b, partners 64 I + a ascending)
template <bool P2, class AF, class CF>
__device__ __forceinline__ void ax_sum_col(const double* tile, uint32_t I, uint32_t J, uint32_t n, uint32_t lane, AF ACC, CF C) {
    const uint32_t j = 64 * J + lane;
    if (j >= n) return;
    double acc = ACC(j);
    const double cj = P2 ? C(j) : 0.0;
    for (uint32_t a = 0; a < 64; a++) {
        const double v = tile[a * AX_LD + lane];
        if constexpr (P2) acc = acc + (C(64 * I + a) - cj) * v;
        else acc = acc + (1.0 - v);
    }
    ACC(j) = acc;
}

// the documents of a query that has nothing to learn from
__device__ __forceinline__ void ax_zero(const uint32_t* pos, uint32_t n, uint32_t t, uint32_t stride, double* lam, double* wt, float* target) {
    for (uint32_t i = t; i < n; i += stride) {
        const uint32_t p = pos[i];
        lam[p] = 0.0;
        wt[p] = 0.0;
        target[p] = 0.0f;
    }
}

// qorder[q0 .. n_q): queries of at most 64 documents; wave w of block b takes qorder[q0 + 4 b + w].  A wave without a live
// query runs the same barriers over n = 0 documents.
__global__ __launch_bounds__(256) void lambda_grad_approx_wave_kernel(const double* __restrict__ scores, const uint32_t* __restrict__ lm_off,
                                                                      const uint32_t* __restrict__ lm_pos, const uint32_t* __restrict__ qorder,
                                                                      uint32_t q0, uint32_t n_q, const double* __restrict__ gexp,
                                                                      const double* __restrict__ norms, double alpha, double* lam, double* wt,
                                                                      float* target) {
    extern __shared__ double ax_lds[];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u, slot = q0 + blockIdx.x * AX_WAVES + wv;
    double* tile = ax_lds + (size_t)wv * (AX_TILE + 128);
    double* s_l = tile + AX_TILE;
    double* c_l = s_l + 64;
    uint32_t n = 0;
    const uint32_t* pos = lm_pos;
    double norm = 0.0;
    if (slot < n_q) {
        const uint32_t q = qorder[slot], off = lm_off[q];
        n = min(lm_off[q + 1] - off, AX_WAVE_MAX);  // (the launcher sends no longer query here)
        pos = lm_pos + off;
        norm = norms[q];
        if (n < 2 || !(norm > 0.0)) {
            ax_zero(pos, n, lane, 64, lam, wt, target);
            n = 0;
        }
    }
    const uint32_t p = lane < n ? pos[lane] : 0u;
    if (lane < n) s_l[lane] = scores[p];
    __syncthreads();
    auto S = [&](uint32_t i) { return s_l[i]; };
    auto C = [&](uint32_t i) { return c_l[i]; };
    double chain = 0.0;
    auto ACC = [&](uint32_t) -> double& { return chain; };
    ax_fill<1, false>(tile, 0, 0, n, 0, lane, alpha, S);
    __syncthreads();
    ax_sum_diag<false>(tile, 0, n, lane, ACC, C);
    if (lane < n) c_l[lane] = ax_c(chain, gexp[p], norm);
    __syncthreads();  // (every row walk of pass 1 is over before a q becomes a p)
    for (uint32_t d = 1; d <= 32; d++) {  // ax_fill's circulant: every lane converts what it wrote
        const uint32_t o = (lane + d) & 63u, a = min(lane, o), b = max(lane, o);
        if ((d == 32 && lane >= 32) || b >= n) continue;
        const double q = tile[a * AX_LD + b];
        tile[a * AX_LD + b] = q * (1.0 - q);
    }
    __syncthreads();
    chain = 0.0;
    ax_sum_diag<true>(tile, 0, n, lane, ACC, C);
    if (lane < n) {
        const double l = alpha * chain;
        lam[p] = l;
        wt[p] = 0.0;
        target[p] = (float)l;
    }
}

// one query of more than 64 documents by the whole workgroup.  STAGED: n <= AX_STAGE, and s, pass 1's chain (then c) and pass
// 2's chain live in LDS.  Otherwise the chains live in wt (r, then c) and lam, and before a tile is filled waves 2 and 3 copy
// the scores, waves 0 and 1 the c, of its two blocks to LDS (slot 64 + b for block J, slot a for block I), so that no chain
// step waits for memory.
template <bool STAGED>
__device__ __forceinline__ void ax_group_query(double* lds, const double* __restrict__ scores, const uint32_t* __restrict__ pos, uint32_t n,
                                               const double* __restrict__ gexp, double norm, double alpha, double* lam, double* wt, float* target) {
    const uint32_t tid = threadIdx.x, wv = tid >> 6, lane = tid & 63u, nblk = (n + 63u) / 64u;
    double* tile = lds;
    double* s_l = lds + AX_TILE;
    double* r_l = s_l + AX_STAGE;
    double* a_l = r_l + AX_STAGE;
    uint32_t I = 0, J = 0;
    auto slot = [&](uint32_t i) { return STAGED ? i : ((i >> 6) == J ? 64u : 0u) + (i & 63u); };
    auto S = [&](uint32_t i) { return s_l[slot(i)]; };
    auto C = [&](uint32_t i) { return r_l[slot(i)]; };
    auto R = [&](uint32_t i) -> double& {  // pass 1's chain, then c
        if constexpr (STAGED) return r_l[i];
        else return wt[pos[i]];
    };
    auto A = [&](uint32_t i) -> double& {  // pass 2's chain
        if constexpr (STAGED) return a_l[i];
        else return lam[pos[i]];
    };
    // the blocks of tile (I, J) to LDS (nothing to do when the query is staged); with_c: pass 2
    auto stage_blocks = [&](bool with_c) {
        if constexpr (!STAGED) {
            const uint32_t i = 64 * ((wv & 1u) ? J : I) + lane;
            if (i < n && (wv >= 2 || with_c)) {
                const uint32_t p = pos[i];
                if (wv >= 2) s_l[slot(i)] = scores[p];
                else r_l[slot(i)] = wt[p];
            }
            __syncthreads();
        }
    };
    for (uint32_t i = tid; i < n; i += 256) {
        if constexpr (STAGED) s_l[i] = scores[pos[i]];
        R(i) = 0.0;
    }
    __syncthreads();
    for (J = 0; J < nblk; J++) {
        for (I = 0; I <= J; I++) {
            stage_blocks(false);
            ax_fill<AX_WAVES, false>(tile, I, J, n, wv, lane, alpha, S);
            __syncthreads();
            if (I == J) {
                if (wv == 0) ax_sum_diag<false>(tile, I, n, lane, R, C);
            } else if (wv == 0) {
                ax_sum_row<false>(tile, I, J, n, lane, R, C);
            } else if (wv == 1) {
                ax_sum_col<false>(tile, I, J, n, lane, R, C);
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < n; i += 256) {
        R(i) = ax_c(R(i), gexp[pos[i]], norm);
        A(i) = 0.0;
    }
    __syncthreads();
    for (J = 0; J < nblk; J++) {
        for (I = 0; I <= J; I++) {
            stage_blocks(true);
            ax_fill<AX_WAVES, true>(tile, I, J, n, wv, lane, alpha, S);
            __syncthreads();
            if (I == J) {
                if (wv == 0) ax_sum_diag<true>(tile, I, n, lane, A, C);
            } else if (wv == 0) {
                ax_sum_row<true>(tile, I, J, n, lane, A, C);
            } else if (wv == 1) {
                ax_sum_col<true>(tile, I, J, n, lane, A, C);
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < n; i += 256) {
        const uint32_t p = pos[i];
        const double l = alpha * A(i);
        lam[p] = l;
        wt[p] = 0.0;
        target[p] = (float)l;
    }
}

// qorder[0 .. gridDim.x): the queries of more than 64 documents, longest first; block b takes qorder[b]
__global__ __launch_bounds__(256) void lambda_grad_approx_kernel(const double* __restrict__ scores, const uint32_t* __restrict__ lm_off,
                                                                 const uint32_t* __restrict__ lm_pos, const uint32_t* __restrict__ qorder,
                                                                 const double* __restrict__ gexp, const double* __restrict__ norms, double alpha,
                                                                 double* lam, double* wt, float* target) {
    extern __shared__ double ax_lds[];
    const uint32_t q = qorder[blockIdx.x];
    const uint32_t off = lm_off[q], n = lm_off[q + 1] - off;
    const uint32_t* pos = lm_pos + off;
    const double norm = norms[q];
    if (n < 2 || !(norm > 0.0)) {  // (the whole workgroup: none of it reaches a barrier)
        ax_zero(pos, n, threadIdx.x, 256, lam, wt, target);
        return;
    }
    if (n <= AX_STAGE) ax_group_query<true>(ax_lds, scores, pos, n, gexp, norm, alpha, lam, wt, target);
    else ax_group_query<false>(ax_lds, scores, pos, n, gexp, norm, alpha, lam, wt, target);
}
