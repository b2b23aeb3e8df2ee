// Part of device.hip (single translation unit; see that file's header).  Resampling per-query values (DESIGN.md section 15):
// the paired bootstrap and the per-query permutation of a table V[Q][M] (row q: one query's value under each of M systems).
// resample.hpp states the streams and the sum's shape; tests/resample_model.py restates both kernels in numpy and the device
// is held to it bit for bit.
//
//   lane = trial.  ceil(T / 64) waves; a lane with t >= T writes nothing.  No atomics: trial t writes out[t * M .. t * M + M).
//   SUM            every lane carries, per column, a segment accumulator and a total: RESAMPLE_SEG = MEAN_SEG consecutive terms
//                  are added one after the other from +0.0, the segments' partials one after the other from +0.0 (the shape of
//                  the mean over queries, kernels_metric.inc); the division by Q is the one rounded f64 division.
//   counter        term k of trial t hashes K + G (t Q + k + 1): the lane keeps the sum and adds G per term.

constexpr uint32_t RESAMPLE_SEG = MEAN_SEG;
static_assert(RESAMPLE_SEG == frresample::SEG, "the host's SUM and the kernels' share one segment length");

// the splitmix64 finaliser of a counter already advanced (xe_gamma's, kernels_xendcg.inc, without its conversion)
__device__ __forceinline__ uint64_t resample_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// Bootstrap: boot[t][c] = SUM_k V[i(t,k)][c] / Q, i(t,k) = ((mix(K_B + G (t Q + k + 1)) >> 32) Q) >> 32.  One draw serves
// every column.  The draws of U consecutive terms do not depend on each other, so their U rows are fetched together and
// then added in order: the gathers' latency is paid once per U terms.  LDS = true: the workgroup first copies V into LDS
// (the launcher has checked Q M 8 <= frresample::LDS_BYTES) and the rows are gathered from there.
template <int M, bool LDS>
__global__ __launch_bounds__(LDS ? frresample::LDS_BLOCK : 64) void resample_boot_kernel(const double* __restrict__ V, uint32_t Q, uint32_t T, uint64_t key,
                                                                                         double* __restrict__ boot) {
    constexpr int U = M <= 2 ? 8 : M <= 4 ? 4 : 2;
    static_assert(RESAMPLE_SEG % U == 0, "a segment is a whole number of fetch groups");
    extern __shared__ double resample_lds[];
    const double* rows = V;
    if constexpr (LDS) {
        const size_t cells = (size_t)Q * M;
        for (size_t i = threadIdx.x; i < cells; i += blockDim.x) resample_lds[i] = V[i];
        __syncthreads();
        rows = resample_lds;
    }
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    constexpr uint64_t G = frresample::GOLDEN;
    uint64_t ctr = key + G * ((uint64_t)t * Q + 1ull);
    double seg[M], tot[M];
#pragma unroll
    for (int c = 0; c < M; c++) seg[c] = 0.0, tot[c] = 0.0;
    uint32_t k = 0;
    while (k < Q) {
        const uint32_t left = Q - k;
        const uint32_t len = left < RESAMPLE_SEG ? left : RESAMPLE_SEG;
        uint32_t j = 0;
        for (; j + U <= len; j += U) {
            double v[U][M];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t i = __umulhi((uint32_t)(resample_mix(ctr) >> 32), Q);
                ctr += G;
                const double* row = rows + (size_t)i * M;
#pragma unroll
                for (int c = 0; c < M; c++) v[u][c] = row[c];
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int c = 0; c < M; c++) seg[c] += v[u][c];
        }
        for (; j < len; j++) {
            const uint32_t i = __umulhi((uint32_t)(resample_mix(ctr) >> 32), Q);
            ctr += G;
            const double* row = rows + (size_t)i * M;
#pragma unroll
            for (int c = 0; c < M; c++) seg[c] += row[c];
        }
#pragma unroll
        for (int c = 0; c < M; c++) tot[c] += seg[c], seg[c] = 0.0;
        k += len;
    }
#pragma unroll
    for (int c = 0; c < M; c++) boot[(size_t)t * M + c] = tot[c] / (double)Q;
}

template <int M>
struct ResampleFactorial {
    static constexpr uint32_t value = (uint32_t)M * ResampleFactorial<M - 1>::value;
};
template <>
struct ResampleFactorial<1> {
    static constexpr uint32_t value = 1;
};

// One step of the decode, i = I down to 1: j = r mod (i + 1), r = r div (i + 1), swap entries i and j.  The entries are the
// row's values themselves (w[c] = V[q][p[c]] holds before and after a swap of p), and the swap is made of selects over the
// compile-time positions 0..i: an array indexed by j would live in scratch.
template <int M, int I>
__device__ __forceinline__ void resample_perm_step(double (&w)[M], uint32_t& r) {
    if constexpr (I >= 1) {
        const uint32_t j = r % (uint32_t)(I + 1);
        r = r / (uint32_t)(I + 1);
        const double top = w[I];
        double got = top;
#pragma unroll
        for (int s = 0; s < I; s++) {
            const bool hit = j == (uint32_t)s;
            got = hit ? w[s] : got;
            w[s] = hit ? top : w[s];
        }
        w[I] = got;
        resample_perm_step<M, I - 1>(w, r);
    }
}

// Permutation: perm[t][c] = SUM_q V[q][p[c]] / Q, p the permutation the Lehmer code r = ((mix(K_P + G (t Q + q + 1)) >> 32) M!)
// >> 32 decodes to.  Every lane of a wave reads the same row q: the loads are wave-uniform.
template <int M>
__global__ __launch_bounds__(64) void resample_perm_kernel(const double* __restrict__ V, uint32_t Q, uint32_t T, uint64_t key, double* __restrict__ perm) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    constexpr uint64_t G = frresample::GOLDEN;
    constexpr uint32_t FACT = ResampleFactorial<M>::value;
    uint64_t ctr = key + G * ((uint64_t)t * Q + 1ull);
    double seg[M], tot[M];
#pragma unroll
    for (int c = 0; c < M; c++) seg[c] = 0.0, tot[c] = 0.0;
    uint32_t q = 0;
    while (q < Q) {
        const uint32_t left = Q - q;
        const uint32_t len = left < RESAMPLE_SEG ? left : RESAMPLE_SEG;
        const double* row = V + (size_t)q * M;
        for (uint32_t j = 0; j < len; j++, row += M) {
            uint32_t r = __umulhi((uint32_t)(resample_mix(ctr) >> 32), FACT);
            ctr += G;
            double w[M];
#pragma unroll
            for (int c = 0; c < M; c++) w[c] = row[c];
            resample_perm_step<M, M - 1>(w, r);
#pragma unroll
            for (int c = 0; c < M; c++) seg[c] += w[c];
        }
#pragma unroll
        for (int c = 0; c < M; c++) tot[c] += seg[c], seg[c] = 0.0;
        q += len;
    }
#pragma unroll
    for (int c = 0; c < M; c++) perm[(size_t)t * M + c] = tot[c] / (double)Q;
}
