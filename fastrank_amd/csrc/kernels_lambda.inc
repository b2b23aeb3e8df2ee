// Part of device.hip (single translation unit; see that file's header).  LambdaMART's gradient pass (DESIGN.md section 11):
// the LambdaRank gradient lambda_p and second-derivative weight w_p of every document for the running scores.
//
// One workgroup per query, queries launched longest first (qorder).  The query's documents are staged in its STORED order
// (instance ids ascending: lm_pos lists their positions) -- score, gain, 2^g - 1, instance id, then rank and discount --
// in LDS, or in a per-block global slab when the query does not fit LDS.  Each thread owns documents i = tid, tid + bs, ...
// and walks every partner j = 0..n-1 in stored order with broadcast reads, adding its pair terms to two f64 registers one
// after the other: the association the definition fixes, whatever the block size.
//
//   rank r_i:  partners ahead of i in the RankedInstance order (score desc, gain asc, id asc), counted
//   D(r)    =  1 / log2(r + 2) for r < k (disc[r] = log2(r + 2), the metric kernels' table), 0 beyond; k = n without depth
//   pair (h = higher label, l = lower):  delta = |G_h - G_l| * |D_h - D_l| / Z,  rho = 1 / (1 + exp(sigma (s_h - s_l)))
//            lambda_h += sigma rho delta,  lambda_l -= sigma rho delta,  w_h and w_l += sigma^2 rho (1 - rho) delta
// A query whose norm Z is NaN (no positive label) or not positive gets lambda = w = 0.  -ffp-contract=off (the build's
// flag) keeps every product and sum separately rounded, as written.

constexpr uint32_t LM_STAGE_BYTES = 8 + 8 + 8 + 4 + 4 + 4;  // s, G, D, id, gain, rank per document
constexpr size_t LM_LDS_MAX = (size_t)144 << 10;  // queries of up to 4096 documents are staged in LDS
constexpr uint32_t LM_SLAB_BLOCKS = 1024;           // longer ones: at most this many workgroups per launch, each with a global slab

// ----------------------------------------------------------------------------------------------------------------------
// Objectives (DESIGN.md section 11, "Objectives").  Both kernels below are templates over the objective: LM_OBJ_NDCG is the
// code as it was, statement for statement; under LM_OBJ_MAP / LM_OBJ_MRR only the pair weight delta changes.  A pair
// then is one relevant (gain > 0: h) and one non-relevant document (l), whatever their grades.
//   map   tables over ranks, built once per query over the staging columns NDCG keeps its gains and discounts in (both
//         dead here): relr[r] = the document of rank r is relevant (scattered), c[r] = relevant documents of rank <= r (an
//         integer scan: every thread counts one contiguous stretch, the stretches' offsets come from 256 partial counts),
//         P[r] = sum of 1 / (r' + 1) over the relevant ranks r' <= r: the quotients 256 wide, then ONE thread adds them in
//         rank order (the association the definition fixes; a non-relevant rank adds +0.0, which changes no bit).
//         a = min(r_h, r_l), b = max, up = r_l < r_h:  delta = |(c[a] + up)/(a + 1) - c[b]/(b + 1) + (P[b-1] - P[a])| / R_q
//   mrr   f = the smallest relevant rank, f2 = the next one (two LDS atomicMin reductions).  r_l < f: delta =
//         1/(r_l + 1) - 1/(f + 1); r_h == f: delta = 1/(f + 1) - 1/(min(f2, r_l) + 1); every other pair has delta = 0 and
//         is dropped before its exp, so a query costs about f R + n exponentials, not n^2.
constexpr int LM_OBJ_NDCG = 0, LM_OBJ_MAP = 1, LM_OBJ_MRR = 2;
constexpr uint32_t LM_NO_RANK = 0xFFFFFFFFu;
static_assert(LM_OBJ_NDCG == M_NDCG && LM_OBJ_MAP == M_AP && LM_OBJ_MRR == M_RR, "an objective is spelled as its measure");

struct LmObjective {
    const double* P;    // map: [n] by rank (the G column)
    const uint32_t* c;  // map: [n] by rank (the first half of the D column)
    double rq;          // map: (double)R_q
    uint32_t f, f2;     // mrr: LM_NO_RANK = none
};

// The objective's tables for the staged query; false: the query has nothing to learn from (every thread gets the same
// answer).  part: 256 words of LDS (one per thread).  Called by all threads of the block, after the ranks are known.
template <int OBJ>
__device__ bool lm_objective_tables(uint32_t n, uint32_t tid, uint32_t bs, const float* g, const uint32_t* rk, double* Gcol,
                                    double* Dcol, uint32_t cap, double norm, uint32_t* part, LmObjective& ob) {
    if constexpr (OBJ == LM_OBJ_MAP) {
        double* P = Gcol;
        uint32_t* c = (uint32_t*)Dcol;
        uint32_t* relr = c + cap;
        for (uint32_t i = tid; i < n; i += bs) relr[rk[i]] = g[i] > 0.0f ? 1u : 0u;  // (the ranks are a permutation of 0..n-1)
        __syncthreads();
        const uint32_t seg = (n + bs - 1) / bs, lo = min(tid * seg, n), hi = min(lo + seg, n);
        uint32_t cnt = 0;
        for (uint32_t r = lo; r < hi; r++) cnt += relr[r];
        part[tid] = cnt;
        for (uint32_t r = tid; r < n; r += bs) P[r] = relr[r] ? 1.0 / (double)(r + 1) : 0.0;
        __syncthreads();
        uint32_t run = 0, total = 0;
        for (uint32_t t = 0; t < bs; t++) {
            const uint32_t v = part[t];
            run += t < tid ? v : 0u;
            total += v;
        }
        for (uint32_t r = lo; r < hi; r++) {
            run += relr[r];
            c[r] = run;
        }
        if (tid == 0) {
            double acc = 0.0;
            for (uint32_t r = 0; r < n; r++) {
                acc = acc + P[r];
                P[r] = acc;
            }
        }
        __syncthreads();
        uint32_t R = (uint32_t)norm;
        if (R == 0) R = total;  // no judged count: the list's own (metric_of_ranked's fall-back)
        ob.P = P, ob.c = c, ob.rq = (double)R, ob.f = ob.f2 = LM_NO_RANK;
        return R != 0;
    } else {
        if (tid < 2) part[tid] = LM_NO_RANK;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += bs)
            if (g[i] > 0.0f) atomicMin(&part[0], rk[i]);
        __syncthreads();
        const uint32_t f = part[0];
        for (uint32_t i = tid; i < n; i += bs)
            if (g[i] > 0.0f && rk[i] > f) atomicMin(&part[1], rk[i]);
        __syncthreads();
        ob.P = nullptr, ob.c = nullptr, ob.rq = 0.0, ob.f = f, ob.f2 = part[1];
        return f != LM_NO_RANK;
    }
}

// delta of the pair (h relevant at rank rh, l non-relevant at rank rl); false: delta = 0, the pair is dropped
template <int OBJ>
__device__ __forceinline__ bool lm_objective_delta(const LmObjective& ob, uint32_t rh, uint32_t rl, double& delta) {
    if constexpr (OBJ == LM_OBJ_MAP) {
        const uint32_t a = min(rh, rl), b = max(rh, rl), up = rl < rh ? 1u : 0u;
        const double x = (double)(ob.c[a] + up) / (double)(a + 1);
        const double y = (double)ob.c[b] / (double)(b + 1);
        const double M = (x - y) + (ob.P[b != 0 ? b - 1 : 0] - ob.P[a]);  // (b >= 1: two ranks differ, unless NaN scores broke the order)
        delta = fabs(M) / ob.rq;
        return true;
    } else {
        if (rl < ob.f) {
            delta = 1.0 / (double)(rl + 1) - 1.0 / (double)(ob.f + 1);
            return true;
        }
        if (rh != ob.f) return false;
        const uint32_t m = min(ob.f2, rl);  // (no f2: LM_NO_RANK, so r_l)
        delta = 1.0 / (double)(ob.f + 1) - 1.0 / (double)(m + 1);
        return true;
    }
}

// lambda = w = 0 for the whole query
__device__ __forceinline__ void lm_zero_query(uint32_t n, uint32_t tid, uint32_t bs, const uint32_t* lm_pos, uint32_t off, double* lam,
                                              double* wt, float* target) {
    for (uint32_t i = tid; i < n; i += bs) {
        const uint32_t p = lm_pos[off + i];
        lam[p] = 0.0;
        wt[p] = 0.0;
        target[p] = 0.0f;
    }
}

template <int OBJ>
__global__ __launch_bounds__(256) void lambda_grad_kernel(const double* __restrict__ scores, const uint32_t* __restrict__ lm_off,
                                                          const uint32_t* __restrict__ lm_pos, const uint32_t* __restrict__ qorder,
                                                          uint32_t q_first, const float* __restrict__ gain,
                                                          const double* __restrict__ gexp, const double* __restrict__ disc,
                                                          const uint32_t* __restrict__ perm, const double* __restrict__ norms,
                                                          int64_t depth, double sigma, double* __restrict__ lam,
                                                          double* __restrict__ wt, float* __restrict__ target,
                                                          unsigned char* gslab, uint32_t slab_docs) {
    extern __shared__ double lm_lds[];
    const uint32_t q = qorder[q_first + blockIdx.x];
    const uint32_t off = lm_off[q], n = lm_off[q + 1] - off;
    const uint32_t tid = threadIdx.x, bs = blockDim.x;
    const double z = norms[q];
    if (OBJ == LM_OBJ_NDCG && !(z > 0.0)) {  // NaN (no positive label) or no ideal gain at all: nothing to learn from this query
        for (uint32_t i = tid; i < n; i += bs) {
            const uint32_t p = lm_pos[off + i];
            lam[p] = 0.0;
            wt[p] = 0.0;
            target[p] = 0.0f;
        }
        return;
    }
    const uint32_t cap = gslab != nullptr ? slab_docs : n;
    double* base = gslab != nullptr ? (double*)(gslab + (size_t)blockIdx.x * slab_docs * LM_STAGE_BYTES) : lm_lds;
    double* s = base;
    double* G = s + cap;
    double* D = G + cap;
    uint32_t* id = (uint32_t*)(D + cap);
    float* g = (float*)(id + cap);
    uint32_t* rk = (uint32_t*)(g + cap);
    for (uint32_t i = tid; i < n; i += bs) {
        const uint32_t p = lm_pos[off + i];
        s[i] = scores[p];
        if constexpr (OBJ == LM_OBJ_NDCG) G[i] = gexp[p];
        id[i] = perm[p];
        g[i] = gain[p];
    }
    __syncthreads();
    for (uint32_t i = tid; i < n; i += bs) {
        const double si = s[i];
        const float gi = g[i];
        const uint32_t ii = id[i];
        uint32_t r = 0;
        for (uint32_t j = 0; j < n; j++) {
            const double sj = s[j];
            const float gj = g[j];
            r += (sj > si || (sj == si && (gj < gi || (gj == gi && id[j] < ii)))) ? 1u : 0u;
        }
        rk[i] = r;
    }
    __syncthreads();
    LmObjective ob;
    if constexpr (OBJ == LM_OBJ_NDCG) {
        const uint64_t k = depth < 0 ? (uint64_t)n : (uint64_t)depth;
        for (uint32_t i = tid; i < n; i += bs) D[i] = (uint64_t)rk[i] < k ? 1.0 / disc[rk[i]] : 0.0;
        __syncthreads();
    } else {  // (the measure's depth is not read: the objective has none)
        __shared__ uint32_t part[256];
        if (!lm_objective_tables<OBJ>(n, tid, bs, g, rk, G, D, cap, z, part, ob)) {
            lm_zero_query(n, tid, bs, lm_pos, off, lam, wt, target);
            return;
        }
    }
    const double sigma2 = sigma * sigma;
    for (uint32_t i = tid; i < n; i += bs) {
        const double si = s[i], Gi = OBJ == LM_OBJ_NDCG ? G[i] : 0.0, Di = OBJ == LM_OBJ_NDCG ? D[i] : 0.0;
        const float gi = g[i];
        const bool reli = gi > 0.0f;
        const uint32_t ri = rk[i];
        double l = 0.0, w = 0.0;
        for (uint32_t j = 0; j < n; j++) {
            const float gj = g[j];
            if (OBJ == LM_OBJ_NDCG ? gj == gi : (gj > 0.0f) == reli) continue;
            const bool high = OBJ == LM_OBJ_NDCG ? gi > gj : reli;
            double delta;
            if constexpr (OBJ != LM_OBJ_NDCG) {  // (before the exp: most pairs of mrr have none)
                if (!lm_objective_delta<OBJ>(ob, high ? ri : rk[j], high ? rk[j] : ri, delta)) continue;
            }
            const double diff = high ? si - s[j] : s[j] - si;  // s_h - s_l
            if constexpr (OBJ == LM_OBJ_NDCG) delta = fabs(Gi - G[j]) * fabs(Di - D[j]) / z;
            const double rho = 1.0 / (1.0 + exp(sigma * diff));
            const double t = sigma * rho * delta;
            l = high ? l + t : l - t;
            w = w + sigma2 * rho * (1.0 - rho) * delta;
        }
        const uint32_t p = lm_pos[off + i];
        lam[p] = l;
        wt[p] = w;
        target[p] = (float)l;
    }
}

// ----------------------------------------------------------------------------------------------------------------------
// Truncation level T and per-query normalisation (DESIGN.md section 11, "Truncation and normalisation").
//
// A pair contributes only when the better ranked of its two documents sits in the top T, so a document outside the top T
// has at most T partners and the pass costs n T pair terms instead of n^2.  Staging, ranks and discounts are the
// untruncated kernel's.  Then:
//   top list  the stored-order indices of the documents with rank < T, compacted in stored order (wave ballots) into
//             the staging area of the instance ids, which are dead once the ranks are known; m = min(T, n) entries
//   phase A   every document OUTSIDE the top T walks the top list only: at most T pair terms, one thread per document
//   phase B   the m long chains of the top documents.  32 of them at a time: all 256 threads produce the signed pair
//             terms of 32 chains x 16 partners (fewer chains: more partners, 512 terms either way) into an LDS tile, then
//             the chains' own lanes add their tile row in stored partner order.  A skipped partner's tile entry is +0.0,
//             which changes no bit of a sum that is never -0.0 (DESIGN.md).  The exp runs 256 wide, the dependent adds
//             32 chains wide, and no lane waits for another lane's exp.
//   norm      A_p (the sum of the document's t_pq >= 0, same order) goes to a global scratch, is staged over the dead
//             score column, thread 0 adds S_q sequentially, and every lambda, w of the query is scaled by log2(1 + S_q) / S_q.
// LDS: the staging of lambda_grad_kernel (36 B per document, at most 144 KiB) plus the 8.5 KiB tile and 32 B of counters.
constexpr uint32_t LMT_TILE = 512;             // pair terms produced per step
constexpr uint32_t LMT_CHAINS = 32;            // top documents per group of chains
constexpr uint32_t LMT_TILE_SLOTS = LMT_TILE + LMT_CHAINS;  // rows are padded by one slot: 32 x 17 is the largest tile

template <int OBJ>
__global__ __launch_bounds__(256) void lambda_grad_trunc_kernel(
    const double* __restrict__ scores, const uint32_t* __restrict__ lm_off, const uint32_t* __restrict__ lm_pos,
    const uint32_t* __restrict__ qorder, uint32_t q_first, const float* __restrict__ gain, const double* __restrict__ gexp,
    const double* __restrict__ disc, const uint32_t* __restrict__ perm, const double* __restrict__ norms, int64_t depth,
    double sigma, uint32_t trunc, int normalise, double* lam, double* wt, float* target, double* asum, unsigned char* gslab,
    uint32_t slab_docs) {
    extern __shared__ double lm_lds[];
    __shared__ double2 tile[LMT_TILE_SLOTS];
    __shared__ uint32_t wave_cnt[4];
    __shared__ double scale_f;
    const uint32_t q = qorder[q_first + blockIdx.x];
    const uint32_t off = lm_off[q], n = lm_off[q + 1] - off;
    const uint32_t tid = threadIdx.x, bs = blockDim.x;  // (bs == 256: the tile and the ballots count on it)
    const double z = norms[q];
    if (OBJ == LM_OBJ_NDCG && !(z > 0.0)) {
        for (uint32_t i = tid; i < n; i += bs) {
            const uint32_t p = lm_pos[off + i];
            lam[p] = 0.0;
            wt[p] = 0.0;
            target[p] = 0.0f;
        }
        return;
    }
    const uint32_t cap = gslab != nullptr ? slab_docs : n;
    double* base = gslab != nullptr ? (double*)(gslab + (size_t)blockIdx.x * slab_docs * LM_STAGE_BYTES) : lm_lds;
    double* s = base;
    double* G = s + cap;
    double* D = G + cap;
    uint32_t* id = (uint32_t*)(D + cap);
    float* g = (float*)(id + cap);
    uint32_t* rk = (uint32_t*)(g + cap);
    for (uint32_t i = tid; i < n; i += bs) {
        const uint32_t p = lm_pos[off + i];
        s[i] = scores[p];
        if constexpr (OBJ == LM_OBJ_NDCG) G[i] = gexp[p];
        id[i] = perm[p];
        g[i] = gain[p];
    }
    __syncthreads();
    for (uint32_t i = tid; i < n; i += bs) {
        const double si = s[i];
        const float gi = g[i];
        const uint32_t ii = id[i];
        uint32_t r = 0;
        for (uint32_t j = 0; j < n; j++) {
            const double sj = s[j];
            const float gj = g[j];
            r += (sj > si || (sj == si && (gj < gi || (gj == gi && id[j] < ii)))) ? 1u : 0u;
        }
        rk[i] = r;
    }
    __syncthreads();
    LmObjective ob;
    if constexpr (OBJ == LM_OBJ_NDCG) {
        const uint64_t k = depth < 0 ? (uint64_t)n : (uint64_t)depth;
        for (uint32_t i = tid; i < n; i += bs) D[i] = (uint64_t)rk[i] < k ? 1.0 / disc[rk[i]] : 0.0;
        __syncthreads();
    } else {  // (the measure's depth is not read: the objective has none)
        __shared__ uint32_t part[256];
        if (!lm_objective_tables<OBJ>(n, tid, bs, g, rk, G, D, cap, z, part, ob)) {
            lm_zero_query(n, tid, bs, lm_pos, off, lam, wt, target);
            return;
        }
    }
    // the top list, in stored order, over the ids (dead from here on)
    uint32_t* top = id;
    uint32_t m = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += bs) {
        const uint32_t i = c0 + tid, lane = tid & 63u, wv = tid >> 6;
        const bool in = i < n && rk[i] < trunc;
        const unsigned long long b = __ballot(in ? 1 : 0);
        if (lane == 0) wave_cnt[wv] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = m;
        for (uint32_t x = 0; x < wv; x++) before += wave_cnt[x];
        if (in) top[before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = i;
        m += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    const double sigma2 = sigma * sigma;
    // phase A: a document outside the top T meets the top documents only
    for (uint32_t i = tid; i < n; i += bs) {
        if (rk[i] < trunc) continue;
        const double si = s[i], Gi = OBJ == LM_OBJ_NDCG ? G[i] : 0.0, Di = OBJ == LM_OBJ_NDCG ? D[i] : 0.0;
        const float gi = g[i];
        const bool reli = gi > 0.0f;
        const uint32_t ri = rk[i];
        double l = 0.0, w = 0.0, a = 0.0;
        for (uint32_t c = 0; c < m; c++) {
            const uint32_t j = top[c];
            const float gj = g[j];
            if (OBJ == LM_OBJ_NDCG ? gj == gi : (gj > 0.0f) == reli) continue;
            const bool high = OBJ == LM_OBJ_NDCG ? gi > gj : reli;
            double delta;
            if constexpr (OBJ != LM_OBJ_NDCG) {
                if (!lm_objective_delta<OBJ>(ob, high ? ri : rk[j], high ? rk[j] : ri, delta)) continue;
            }
            const double diff = high ? si - s[j] : s[j] - si;  // s_h - s_l
            if constexpr (OBJ == LM_OBJ_NDCG) delta = fabs(Gi - G[j]) * fabs(Di - D[j]) / z;
            const double rho = 1.0 / (1.0 + exp(sigma * diff));
            const double t = sigma * rho * delta;
            l = high ? l + t : l - t;
            w = w + sigma2 * rho * (1.0 - rho) * delta;
            a = a + t;
        }
        const uint32_t p = lm_pos[off + i];
        lam[p] = l;
        wt[p] = w;
        if (normalise) asum[p] = a;
        else target[p] = (float)l;
    }
    // phase B: the chains of the top documents, LMT_CHAINS at a time
    for (uint32_t a0 = 0; a0 < m; a0 += LMT_CHAINS) {
        const uint32_t rows = min(LMT_CHAINS, m - a0);
        uint32_t cs = 4;  // the tile is (512 >> cs) rows x (1 << cs) partners, the widest that still holds `rows` rows
        while (cs < 9 && (LMT_TILE >> (cs + 1)) >= rows) cs++;
        const uint32_t width = 1u << cs, stride = width + 1;
        double l = 0.0, w = 0.0, a = 0.0;
        for (uint32_t c0 = 0; c0 < n; c0 += width) {
            for (uint32_t e = tid; e < LMT_TILE; e += bs) {
                const uint32_t row = e >> cs, col = e & (width - 1), j = c0 + col;
                if (row >= rows) continue;
                double2 v = make_double2(0.0, 0.0);
                if (j < n) {
                    const uint32_t i = top[a0 + row];
                    const float gi = g[i], gj = g[j];
                    const bool high = OBJ == LM_OBJ_NDCG ? gi > gj : gi > 0.0f;
                    double delta;
                    bool pair = OBJ == LM_OBJ_NDCG ? gj != gi : (gj > 0.0f) != high;
                    if constexpr (OBJ != LM_OBJ_NDCG) pair = pair && lm_objective_delta<OBJ>(ob, high ? rk[i] : rk[j], high ? rk[j] : rk[i], delta);
                    if (pair) {
                        const double si = s[i];
                        const double diff = high ? si - s[j] : s[j] - si;  // s_h - s_l
                        if constexpr (OBJ == LM_OBJ_NDCG) delta = fabs(G[i] - G[j]) * fabs(D[i] - D[j]) / z;
                        const double rho = 1.0 / (1.0 + exp(sigma * diff));
                        const double t = sigma * rho * delta;
                        v.x = high ? t : -t;
                        v.y = sigma2 * rho * (1.0 - rho) * delta;
                    }
                }
                tile[row * stride + col] = v;
            }
            __syncthreads();
            if (tid < rows) {
                const uint32_t cw = min(width, n - c0);
                const double2* r = tile + tid * stride;
                for (uint32_t c = 0; c < cw; c++) {
                    const double2 v = r[c];
                    l = l + v.x;
                    w = w + v.y;
                    a = a + fabs(v.x);
                }
            }
            __syncthreads();
        }
        if (tid < rows) {
            const uint32_t p = lm_pos[off + top[a0 + tid]];
            lam[p] = l;
            wt[p] = w;
            if (normalise) asum[p] = a;
            else target[p] = (float)l;
        }
    }
    if (!normalise) return;
    // S_q: the A_p in stored order, one after the other; then the query's scale
    __syncthreads();  // (phase B's last reads of the scores, and every A_p written)
    for (uint32_t i = tid; i < n; i += bs) s[i] = asum[lm_pos[off + i]];
    __syncthreads();
    if (tid == 0) {
        double S = 0.0;
        for (uint32_t i = 0; i < n; i++) S = S + s[i];
        scale_f = S > 0.0 ? log2(1.0 + S) / S : 1.0;
        wave_cnt[0] = S > 0.0 ? 1u : 0u;
    }
    __syncthreads();
    const double f = scale_f;
    const bool scaled = wave_cnt[0] != 0;
    for (uint32_t i = tid; i < n; i += bs) {
        const uint32_t p = lm_pos[off + i];
        double l = lam[p];
        if (scaled) {
            l = l * f;
            lam[p] = l;
            wt[p] = wt[p] * f;
        }
        target[p] = (float)l;
    }
}
