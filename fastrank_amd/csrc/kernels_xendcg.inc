// Part of device.hip (single translation unit; see that file's header).  LambdaMART's listwise objective (DESIGN.md section 11,
// "Listwise objective"): the cross-entropy NDCG surrogate's gradient lambda_p and weight w_p of every document, O(n) per query.
//
// One WAVE per query, four queries per 256-thread workgroup, queries launched longest first (qorder).  Lane l owns the
// documents i = l, l + 64, ... of the query's STORED order (instance ids ascending: lm_pos lists their positions), which is
// the partial shape the definition fixes for every sum:
//   SUM(x)  P_l = the x_i with i = l (mod 64) added one after the other in ascending i, from +0.0;
//           then P_l = P_l + P_{l+h} for l < h, h = 32, 16, 8, 4, 2, 1 (six __shfl_down steps); the sum is P_0, broadcast.
// No LDS, no block barrier, no atomics: a wave reads its documents, reduces in registers and writes its three outputs.
//
//   gamma_i = (mix(key + 0x9E3779B97F4A7C15 (id_i + 1)) >> 11) 2^-53        mix = the splitmix64 finaliser, id = perm[p]
//   phi_i   = (gexp_i + 1.0) - gamma_i,  Phi = SUM(phi),  inv = 1.0 / Phi     (!(Phi > 0): the query gets zeros)
//   m = max s_i,  e_i = exp(s_i - m),  E = SUM(e),  rho_i = e_i / E,  u_i = 1.0 - rho_i,  Q(x, i) = u_i > 0 ? x / u_i : +0.0
//   t1_i = phi_i inv - rho_i,  a_i = Q(t1_i, i),  S1 = SUM(a)
//   t2_i = rho_i (S1 - a_i),   b_i = Q(t2_i, i),  S2 = SUM(b)
//   t3_i = rho_i (S2 - b_i),   lambda_i = (t1_i + t2_i) + t3_i,  w_i = rho_i u_i
// A query of one document, or whose norm is NaN or not positive, gets lambda = w = 0.  -ffp-contract=off (the build's flag)
// keeps every product and sum separately rounded, as written.
//
// Registers: a lane keeps position, phi and e (then rho) of its first XE_REG documents, so a query of up to 64 XE_REG = 256
// documents reads every input once and calls exp once per document.  A longer query runs the same statements with nothing
// kept: every pass reads score, 2^g - 1 and instance id again and recomputes phi, e, rho, a, b from them.  The recomputed
// values are the same bits (same operands, same operations), so the two paths give one result; the long path costs four exps
// per document instead of one and its re-reads hit the L2.

constexpr int LM_OBJ_XENDCG = 3;
static_assert(LM_OBJ_XENDCG == LM_OBJECTIVE_XENDCG, "the listwise objective's id is the host's");
constexpr uint32_t XE_REG = 4;           // documents per lane kept in registers
constexpr uint32_t XE_WAVES = 4;         // queries per workgroup

__device__ __forceinline__ double xe_gamma(uint64_t key, uint32_t id) {
    uint64_t z = key + 0x9E3779B97F4A7C15ull * ((uint64_t)id + 1ull);
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-53;  // (53 bits: the conversion and the product are exact)
}

// SUM's tree step over the 64 partials; every lane of the wave calls it and gets P_0
__device__ __forceinline__ double xe_tree_sum(double part) {
    for (int h = 32; h >= 1; h >>= 1) part = part + __shfl_down(part, h, 64);  // (lanes >= h hold values nobody reads)
    return __shfl(part, 0, 64);
}

__device__ __forceinline__ double xe_tree_max(double part) {
    for (int h = 32; h >= 1; h >>= 1) part = fmax(part, __shfl_down(part, h, 64));
    return __shfl(part, 0, 64);
}

// one query by one wave.  KEEP: n <= 64 * XE_REG and the lane's documents stay in registers
template <bool KEEP>
__device__ __forceinline__ void xe_query(const double* __restrict__ scores, const uint32_t* __restrict__ pos, uint32_t n, uint32_t lane,
                                         const double* __restrict__ gexp, const uint32_t* __restrict__ perm, uint64_t key,
                                         double* __restrict__ lam, double* __restrict__ wt, float* __restrict__ target) {
    const uint32_t trips = KEEP ? XE_REG : (n + 63u) / 64u;
    uint32_t kp[XE_REG];
    double kphi[XE_REG], krho[XE_REG];  // (krho holds e until E is known)
    // phi and the largest score
    double part = 0.0, m = -INFINITY;
#pragma unroll
    for (uint32_t k = 0; k < trips; k++) {
        const uint32_t i = lane + 64u * k;
        if (i < n) {
            const uint32_t p = pos[i];
            const double s = scores[p];
            const double phi = (gexp[p] + 1.0) - xe_gamma(key, perm[p]);
            if constexpr (KEEP) kp[k] = p, kphi[k] = phi, krho[k] = s;
            part = part + phi;
            m = fmax(m, s);
        }
    }
    const double Phi = xe_tree_sum(part);
    m = xe_tree_max(m);
    if (!(Phi > 0.0)) {  // negative or fractional labels: nothing to learn from this query
        for (uint32_t i = lane; i < n; i += 64u) {
            const uint32_t p = pos[i];
            lam[p] = 0.0;
            wt[p] = 0.0;
            target[p] = 0.0f;
        }
        return;
    }
    const double inv = 1.0 / Phi;
    // E
    part = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < trips; k++) {
        const uint32_t i = lane + 64u * k;
        if (i < n) {
            double e;
            if constexpr (KEEP) e = krho[k] = exp(krho[k] - m);
            else e = exp(scores[pos[i]] - m);
            part = part + e;
        }
    }
    const double E = xe_tree_sum(part);
    // the three passes below share this: the document's phi and rho, from the registers or from memory again
    auto doc = [&](uint32_t k, uint32_t i, uint32_t& p, double& phi, double& rho) {
        if constexpr (KEEP) {
            p = kp[k], phi = kphi[k], rho = krho[k];
        } else {
            p = pos[i];
            phi = (gexp[p] + 1.0) - xe_gamma(key, perm[p]);
            rho = exp(scores[p] - m) / E;
        }
    };
    // S1
    part = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < trips; k++) {
        const uint32_t i = lane + 64u * k;
        if (i < n) {
            if constexpr (KEEP) krho[k] = krho[k] / E;
            uint32_t p;
            double phi, rho;
            doc(k, i, p, phi, rho);
            const double u = 1.0 - rho, t1 = phi * inv - rho;
            part = part + (u > 0.0 ? t1 / u : 0.0);
        }
    }
    const double S1 = xe_tree_sum(part);
    // S2
    part = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < trips; k++) {
        const uint32_t i = lane + 64u * k;
        if (i < n) {
            uint32_t p;
            double phi, rho;
            doc(k, i, p, phi, rho);
            const double u = 1.0 - rho, t1 = phi * inv - rho;
            const double a = u > 0.0 ? t1 / u : 0.0;
            const double t2 = rho * (S1 - a);
            part = part + (u > 0.0 ? t2 / u : 0.0);
        }
    }
    const double S2 = xe_tree_sum(part);
    // lambda, w
#pragma unroll
    for (uint32_t k = 0; k < trips; k++) {
        const uint32_t i = lane + 64u * k;
        if (i < n) {
            uint32_t p;
            double phi, rho;
            doc(k, i, p, phi, rho);
            const double u = 1.0 - rho, t1 = phi * inv - rho;
            const double a = u > 0.0 ? t1 / u : 0.0;
            const double t2 = rho * (S1 - a);
            const double b = u > 0.0 ? t2 / u : 0.0;
            const double t3 = rho * (S2 - b);
            const double l = (t1 + t2) + t3;
            lam[p] = l;
            wt[p] = rho * u;
            target[p] = (float)l;
        }
    }
}

// qorder[n_q]: the queries this launch visits, longest first; wave w of block b takes qorder[4 b + w]
__global__ __launch_bounds__(256) void lambda_grad_xe_kernel(const double* __restrict__ scores, const uint32_t* __restrict__ lm_off,
                                                             const uint32_t* __restrict__ lm_pos, const uint32_t* __restrict__ qorder,
                                                             uint32_t n_q, const double* __restrict__ gexp,
                                                             const uint32_t* __restrict__ perm, const double* __restrict__ norms,
                                                             uint64_t key, double* __restrict__ lam, double* __restrict__ wt,
                                                             float* __restrict__ target) {
    const uint32_t slot = blockIdx.x * XE_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (slot >= n_q) return;  // (the whole wave: no lane of it reaches a shuffle)
    const uint32_t q = qorder[slot];
    const uint32_t off = lm_off[q], n = lm_off[q + 1] - off;
    const uint32_t* pos = lm_pos + off;
    if (n < 2 || !(norms[q] > 0.0)) {  // one document, or NaN (no positive label) / no ideal gain: the NDCG kernel's rule
        for (uint32_t i = lane; i < n; i += 64u) {
            const uint32_t p = pos[i];
            lam[p] = 0.0;
            wt[p] = 0.0;
            target[p] = 0.0f;
        }
        return;
    }
    if (n <= 64u * XE_REG) xe_query<true>(scores, pos, n, lane, gexp, perm, key, lam, wt, target);
    else xe_query<false>(scores, pos, n, lane, gexp, perm, key, lam, wt, target);
}
