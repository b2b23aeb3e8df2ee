// Part of device.hip (single translation unit; see that file's header).  General sort evaluator and the fixed-shape mean reduction.
// a precedes b in the reference order?  Positions are in reverse tie-break layout, so among equal
// scores the HIGHER position ranks first (src/evaluators.rs:34-49).  Invalid (padding) keys last.
__device__ __forceinline__ bool key_before(double sa, uint32_t ia, double sb, uint32_t ib) {
    if (ia == IDX_INVALID) return false;
    if (ib == IDX_INVALID) return true;
    if (sa > sb) return true;
    if (sa < sb) return false;
    return ia > ib;
}

// General evaluator for one (query, score slot): bitonic sort + metric (NDCG, AP, RR in the reference's summation order; DCG,
// precision, recall, success and ERR as measures_host.hpp defines them -- at a cut-off of 1 .. 64 metric_topk_kernel,
// kernels_metric_topk.inc, gives the same bytes without the sort).
// dynamic LDS: double keys[npad]; uint32 idx[npad]; (npad = pow2 >= longest query of the size class).
// Queries too long for LDS (> 8192 documents) sort in a global scratch slab instead (gkeys/gidx,
// one slab of npad_max entries per block): same code, one block per query, __syncthreads() orders
// the block's own global writes.
__global__ __launch_bounds__(256) void metric_sort_kernel(
    const double* __restrict__ scores, uint32_t np, const uint32_t* __restrict__ qstart,
    const uint32_t* __restrict__ qlen, const uint32_t* __restrict__ qtight, const double* __restrict__ gexp,
    const float* __restrict__ gain, const double* __restrict__ disc, const double* __restrict__ norms, int measure,
    int depth, uint32_t B, double* __restrict__ M, uint32_t* __restrict__ rank_out, const uint32_t* __restrict__ perm,
    int* __restrict__ flags, uint32_t npad_max, const uint32_t* __restrict__ qlist, uint32_t b_off,
    double* gkeys, uint32_t* gidx) {
    extern __shared__ double lds_raw[];
    double* keys = lds_raw;
    uint32_t* idx = (uint32_t*)(keys + npad_max);
    if (gkeys != nullptr) {
        const size_t slab = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * npad_max;
        keys = gkeys + slab;
        idx = gidx + slab;
    }
    // queries are launched per size class so that the LDS footprint matches the query length
    const uint32_t q = qlist[blockIdx.x], b = blockIdx.y + b_off, tid = threadIdx.x, nt = blockDim.x;
    const uint32_t base = qstart[q], n = qlen[q];
    uint32_t npad = 1;
    while (npad < n) npad <<= 1;
    const double* sc = scores + (size_t)b * np + base;
    bool nan_seen = false;
    for (uint32_t i = tid; i < npad; i += nt) {
        if (i < n) {
            double s = sc[i];
            nan_seen |= (s != s);
            keys[i] = s;
            idx[i] = i;
        } else {
            keys[i] = 0.0;
            idx[i] = IDX_INVALID;
        }
    }
    if (nan_seen) atomicOr(flags, FLAG_NAN_SCORE);
    __syncthreads();
    for (uint32_t k = 2; k <= npad; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < (npad >> 1); t += nt) {
                uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                uint32_t l = i | j;
                bool up = (i & k) == 0;
                double si = keys[i], sl = keys[l];
                uint32_t ii = idx[i], il = idx[l];
                bool swap = up ? key_before(sl, il, si, ii) : key_before(si, ii, sl, il);
                if (swap) {
                    keys[i] = sl;
                    keys[l] = si;
                    idx[i] = il;
                    idx[l] = ii;
                }
            }
            __syncthreads();
        }
    }
    if (rank_out != nullptr && b == 0) {
        const uint32_t tb = qtight[q];
        for (uint32_t i = tid; i < n; i += nt) rank_out[tb + i] = perm[base + idx[i]];
    }
    double result = 0.0;
    if (measure == M_NDCG) {
        // src/evaluators.rs:255-272,350-380: terms in rank order, sequential sum from 0.0
        uint32_t L = depth >= 0 ? ((uint32_t)depth < n ? (uint32_t)depth : n) : n;
        for (uint32_t i = tid; i < L; i += nt) keys[i] = gexp[base + idx[i]] / disc[i];
        __syncthreads();
        if (tid == 0) {
            double norm = norms[q];
            if (norm == norm) {
                double dcg = 0.0;
                for (uint32_t i = 0; i < L; i++) dcg = dcg + keys[i];
                if (dcg > norm) atomicOr(flags, FLAG_ACTUAL_GT_IDEAL);
                result = dcg / norm;
            }
        }
    } else if (measure >= M_DCG) {
        // the five measures of measures_host.hpp, its operands in its order
        const uint32_t L = depth >= 0 ? ((uint32_t)depth < n ? (uint32_t)depth : n) : n;
        const double norm = norms[q];
        if (measure == M_DCG) {
            for (uint32_t i = tid; i < L; i += nt) keys[i] = gexp[base + idx[i]] / disc[i];
        } else if (measure == M_ERR) {
            for (uint32_t i = tid; i < L; i += nt) keys[i] = gain[base + idx[i]] > 0.0f ? gexp[base + idx[i]] / norm : 0.0;
        } else {
            // (recall's fallback counts the whole list)
            for (uint32_t i = tid; i < n; i += nt) keys[i] = gain[base + idx[i]] > 0.0f ? 1.0 : 0.0;
        }
        __syncthreads();
        if (tid == 0) {
            if (measure == M_DCG) {
                for (uint32_t i = 0; i < L; i++) result = result + keys[i];
            } else if (measure == M_ERR) {
                double p = 1.0;
                for (uint32_t i = 0; i < L; i++) {
                    const double R = keys[i];
                    result = result + (p * R) / (double)(i + 1);
                    p = p * (1.0 - R);
                }
            } else {
                uint32_t c = 0;
                for (uint32_t i = 0; i < L; i++) c += keys[i] != 0.0;
                if (measure == M_PRECISION) {
                    result = (double)c / norm;
                } else if (measure == M_SUCCESS) {
                    result = c != 0 ? 1.0 : 0.0;
                } else {
                    uint32_t num_rel = (uint32_t)norm;
                    if (num_rel == 0)
                        for (uint32_t i = 0; i < n; i++) num_rel += keys[i] != 0.0;
                    if (num_rel != 0) result = (double)c / (double)num_rel;
                }
            }
        }
    } else {
        // relevance flags in rank order (src/evaluators.rs:94-96 is_relevant: gain > 0)
        for (uint32_t i = tid; i < n; i += nt) keys[i] = gain[base + idx[i]] > 0.0f ? 1.0 : 0.0;
        __syncthreads();
        if (tid == 0) {
            if (measure == M_AP) {
                // src/evaluators.rs:422-447, step 1: recall_points at every relevant rank
                uint32_t c = 0;
                for (uint32_t i = 0; i < n; i++) {
                    c += keys[i] != 0.0;
                    idx[i] = keys[i] != 0.0 ? c : 0u;
                }
            } else if (measure == M_RR) {
                // src/evaluators.rs:239-252
                for (uint32_t i = 0; i < n; i++) {
                    if (keys[i] != 0.0) {
                        result = 1.0 / (double)(i + 1);
                        break;
                    }
                }
            }
        }
        if (measure == M_AP) {
            __syncthreads();
            // step 2 (all threads): precision at each relevant rank, the reference's operands exactly
            for (uint32_t i = tid; i < n; i += nt)
                if (idx[i]) keys[i] = (double)(int)idx[i] / (double)(i + 1);
            __syncthreads();
            if (tid == 0) {
                // step 3: ordered sum in rank order, then / num_relevant
                uint32_t num_rel = (uint32_t)norms[q];
                uint32_t in_list = 0;
                double sum_precision = 0.0;
                for (uint32_t i = 0; i < n; i++) {
                    if (idx[i]) {
                        sum_precision += keys[i];
                        in_list++;
                    }
                }
                if (num_rel == 0) num_rel = in_list;
                if (num_rel != 0) result = sum_precision / (double)num_rel;
            }
        }
    }
    if (tid == 0) M[(size_t)q * B + b] = result;
}

// Mean over queries with a FIXED two-level summation shape (the reference sums in a fresh
// HashMap's iteration order, i.e. unspecified: src/evaluators.rs:173-184 + dense_dataset.rs:96-109):
//   partial[s][c] = sequential sum of M[q][c] over segment s = queries [s*MEAN_SEG, (s+1)*MEAN_SEG)
//   mean[c]       = (sequential sum of partial[s][c] over s) / nq
// For nq <= MEAN_SEG this is the plain sequential sum in query order.
constexpr uint32_t MEAN_SEG = 256;

__global__ __launch_bounds__(64) void segment_sum_kernel(const double* __restrict__ M, uint32_t ldm, uint32_t ncols,
                                                         uint32_t nq, double* __restrict__ partial) {
    const uint32_t c = blockIdx.y * blockDim.x + threadIdx.x;
    const uint32_t s = blockIdx.x;
    if (c >= ncols) return;
    const uint32_t q0 = s * MEAN_SEG;
    const uint32_t q1 = (q0 + MEAN_SEG < nq) ? q0 + MEAN_SEG : nq;
    const double* p = M + (size_t)q0 * ldm + c;
    double sum = 0.0;
    uint32_t q = q0;
    for (; q + 16 <= q1; q += 16) {
        double v[16];
#pragma unroll
        for (int t = 0; t < 16; t++) v[t] = p[(size_t)t * ldm];
#pragma unroll
        for (int t = 0; t < 16; t++) sum += v[t];
        p += (size_t)16 * ldm;
    }
    for (; q < q1; q++) {
        sum += *p;
        p += ldm;
    }
    partial[(size_t)s * ldm + c] = sum;
}

// `div` = number of queries, or 1 when the caller wants the sum itself (query-sharded training adds
// the shards' sums in rank order before dividing by the global query count).
// tail_count / tail_flags (optional): a line search's redo counter and error bits, copied behind the means (means[ldm],
// means[ldm + 1] as raw 64-bit words) so that ONE copy brings a tick's results back instead of three; tail_groups
// (optional, with tail_count): 2 * (ldm / 64) per-group counts -- redo pairs of every group, then insertion-chain runs of
// every group -- as 32-bit words from means[ldm + 2] on.
__host__ __device__ constexpr size_t mean_tail_words(size_t ldm) { return 2 + ldm / 64; }
__global__ void final_mean_kernel(const double* __restrict__ partial, uint32_t ldm, uint32_t ncols, uint32_t nseg,
                                  uint32_t div, double* __restrict__ means, const unsigned long long* __restrict__ tail_count,
                                  const int* __restrict__ tail_flags, double* __restrict__ host_copy,
                                  const uint32_t* __restrict__ tail_groups) {
    // host_copy (optional): page-locked host memory the results are ALSO written to, straight from this kernel -- a tick's
    // results then reach the host without a copy of their own (a one-workgroup copy kernel queued behind another set's
    // verify grid waited up to 0.7 ms for a wave slot in the round-4 timelines)
    uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && tail_count != nullptr) {
        const unsigned long long w0 = *tail_count, w1 = (unsigned long long)(unsigned int)*tail_flags;
        reinterpret_cast<unsigned long long*>(means)[ldm] = w0;
        reinterpret_cast<unsigned long long*>(means)[ldm + 1] = w1;
        if (host_copy != nullptr) {
            reinterpret_cast<unsigned long long*>(host_copy)[ldm] = w0;
            reinterpret_cast<unsigned long long*>(host_copy)[ldm + 1] = w1;
        }
    }
    if (tail_groups != nullptr && c < 2 * (ldm / 64)) {
        const uint32_t v = tail_groups[c];
        reinterpret_cast<uint32_t*>(means + ldm + 2)[c] = v;
        if (host_copy != nullptr) reinterpret_cast<uint32_t*>(host_copy + ldm + 2)[c] = v;
    }
    if (c >= ncols) return;
    // (the additions stay sequential in segment order; the loads do not depend on them: sixteen in flight -- the plain
    // loop waited for every load in turn, 45-50 us for the 122 segments of the 30K shape on the critical path of a tick)
    double sum = 0.0;
    uint32_t s = 0;
    const double* p = partial + c;
    for (; s + 16 <= nseg; s += 16) {
        double v[16];
#pragma unroll
        for (int t = 0; t < 16; t++) v[t] = p[(size_t)(s + t) * ldm];
#pragma unroll
        for (int t = 0; t < 16; t++) sum += v[t];
    }
    for (; s < nseg; s++) sum += p[(size_t)s * ldm];
    const double mean = div ? sum / (double)div : 0.0;
    means[c] = mean;
    if (host_copy != nullptr) host_copy[c] = mean;
}

// The same mean over two SUBSETS of the queries at once: LambdaMART's training and held-out queries (DESIGN.md section 11,
// "Validation and early stopping").  idx = the first subset's queries (n_a, ascending), then the second's (n_b); a
// subset's mean has the shape above over its COMPACTED list of per-query values (column 0 of M):
//   partial[s] = sequential sum of segment s = MEAN_SEG consecutive entries of the compacted list
//   mean       = (sequential sum of the subset's partials) / the subset's size
// One workgroup per segment (nseg_a of the first subset, then the second's): the gather goes through LDS, one value per
// thread, and one thread adds the values in order.
__global__ __launch_bounds__(MEAN_SEG) void subset_segment_sum_kernel(const double* __restrict__ M, uint32_t ldm,
                                                                      const uint32_t* __restrict__ idx, uint32_t n_a, uint32_t n_b,
                                                                      uint32_t nseg_a, double* __restrict__ partial) {
    __shared__ double v[MEAN_SEG];
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    const bool second = s >= nseg_a;
    const uint32_t base = second ? n_a : 0u, n = second ? n_b : n_a;
    const uint32_t i0 = (second ? s - nseg_a : s) * MEAN_SEG;
    const uint32_t cnt = i0 < n ? (n - i0 < MEAN_SEG ? n - i0 : MEAN_SEG) : 0u;
    if (tid < cnt) v[tid] = M[(size_t)idx[base + i0 + tid] * ldm];
    __syncthreads();
    if (tid != 0) return;
    double sum = 0.0;
    for (uint32_t i = 0; i < cnt; i++) sum += v[i];
    partial[s] = sum;
}

// means[0] / means[1]: the first / second subset's mean.  One workgroup of two waves: a wave per subset, its partials
// staged in LDS a stretch at a time, its first lane adding them in segment order.
__global__ __launch_bounds__(128) void subset_final_mean_kernel(const double* __restrict__ partial, uint32_t nseg_a, uint32_t nseg_b,
                                                                uint32_t n_a, uint32_t n_b, double* __restrict__ means) {
    __shared__ double v[2][64];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double* p = partial + (w ? nseg_a : 0u);
    const uint32_t nseg = w ? nseg_b : nseg_a, div = w ? n_b : n_a;
    const uint32_t rounds = ((nseg_a > nseg_b ? nseg_a : nseg_b) + 63) / 64;  // (both waves reach every barrier)
    double sum = 0.0;
    for (uint32_t r = 0; r < rounds; r++) {
        const uint32_t s0 = r * 64;
        if (s0 + lane < nseg) v[w][lane] = p[s0 + lane];
        __syncthreads();
        if (lane == 0)
            for (uint32_t i = 0; i < 64 && s0 + i < nseg; i++) sum += v[w][i];
        __syncthreads();
    }
    if (lane == 0) means[w] = div ? sum / (double)div : 0.0;
}
