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
    if (!(z > 0.0)) {  // NaN (no positive label) or no ideal gain at all: nothing to learn from this query
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
        G[i] = gexp[p];
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
    const uint64_t k = depth < 0 ? (uint64_t)n : (uint64_t)depth;
    for (uint32_t i = tid; i < n; i += bs) D[i] = (uint64_t)rk[i] < k ? 1.0 / disc[rk[i]] : 0.0;
    __syncthreads();
    const double sigma2 = sigma * sigma;
    for (uint32_t i = tid; i < n; i += bs) {
        const double si = s[i], Gi = G[i], Di = D[i];
        const float gi = g[i];
        double l = 0.0, w = 0.0;
        for (uint32_t j = 0; j < n; j++) {
            const float gj = g[j];
            if (gj == gi) continue;
            const bool high = gi > gj;
            const double diff = high ? si - s[j] : s[j] - si;  // s_h - s_l
            const double delta = fabs(Gi - G[j]) * fabs(Di - D[j]) / z;
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
