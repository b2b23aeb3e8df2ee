// Part of device.hip (single translation unit; see that file's header).  The five cut-off measures of measures_host.hpp
// (DCG, precision, recall, success, ERR at a depth of 1 .. 64) by SELECTION instead of a sort: DESIGN.md section 17.
//
// One wave per (query, slot); lane l owns documents l, l + 64, ...  A round finds the first key in the reference order
// (key_before: score descending, then the HIGHER position) that the previous round's winner strictly precedes: every lane
// holds the best of its own documents, a six-step butterfly picks the wave's, and only the lane that owned the winner looks
// for its next best.  Positions are unique, so the order is total and the winners of rounds 0 .. k - 1 are the first k
// entries of metric_sort_kernel's sorted list.  Winner r stays in lane r (hence k <= 64); the measure is then added in
// rank order with the operands of measures_host.hpp.  No LDS, no scratch: a query of any length.
constexpr uint32_t TOPK_WAVES = 4;  // (query, slot) pairs per workgroup
constexpr uint32_t TOPK_CACHE = 4;  // a lane's first documents stay in registers: queries of up to 256 are read once

__device__ __forceinline__ double wave_first(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

__global__ __launch_bounds__(64 * TOPK_WAVES) void metric_topk_kernel(
    const double* __restrict__ scores, uint32_t np, const uint32_t* __restrict__ qstart, const uint32_t* __restrict__ qlen,
    const double* __restrict__ gexp, const float* __restrict__ gain, const double* __restrict__ disc,
    const double* __restrict__ norms, int measure, uint32_t depth, uint32_t B, double* __restrict__ M, int* __restrict__ flags,
    const uint32_t* __restrict__ qlist, uint32_t count) {
    const uint32_t lane = threadIdx.x & 63, w = blockIdx.x * TOPK_WAVES + (threadIdx.x >> 6);
    if (w >= count) return;  // (a whole wave: nothing below waits for another wave)
    const uint32_t q = qlist[w], b = blockIdx.y;
    const uint32_t base = qstart[q], n = qlen[q];
    const double* sc = scores + (size_t)b * np + base;
    const double norm = norms[q];
    const uint32_t K = depth < n ? depth : n;
    const bool count_all = measure == M_RECALL && (uint32_t)norm == 0;  // recall's fallback: the whole list's own count

    // first scan: every document once -- NaN scores, the fallback count, the lane's best
    double cs[TOPK_CACHE];
    bool nan_seen = false;
    uint32_t own_rel = 0;
    double bs = 0.0;
    uint32_t bi = IDX_INVALID;
#pragma unroll
    for (uint32_t j = 0; j < TOPK_CACHE; j++) {
        const uint32_t i = lane + 64 * j;
        cs[j] = i < n ? sc[i] : 0.0;
    }
#pragma unroll
    for (uint32_t j = 0; j < TOPK_CACHE; j++) {
        const uint32_t i = lane + 64 * j;
        if (i < n) {
            const double s = cs[j];
            nan_seen |= (s != s);
            if (count_all) own_rel += gain[base + i] > 0.0f;
            if (key_before(s, i, bs, bi)) bs = s, bi = i;
        }
    }
    for (uint32_t i = lane + 64 * TOPK_CACHE; i < n; i += 64) {
        const double s = sc[i];
        nan_seen |= (s != s);
        if (count_all) own_rel += gain[base + i] > 0.0f;
        if (key_before(s, i, bs, bi)) bs = s, bi = i;
    }
    if (nan_seen) atomicOr(flags, FLAG_NAN_SCORE);

    uint32_t mine = 0;  // lane r < L: the position at rank r
    uint32_t L = 0;
    for (; L < K; L++) {
        double ws = bs;
        uint32_t wi = bi;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double os = __shfl_xor(ws, off);
            const uint32_t oi = __shfl_xor(wi, off);
            if (key_before(os, oi, ws, wi)) ws = os, wi = oi;
        }
        // (lanes agree under a total order; NaN scores, already flagged, must not make the loop diverge)
        wi = __builtin_amdgcn_readfirstlane(wi);
        ws = wave_first(ws);
        if (wi == IDX_INVALID) break;  // no candidate left
        if (lane == L) mine = wi;
        if ((wi & 63) == lane && L + 1 < K) {
            // the winner's lane: the best of its documents that the winner strictly precedes
            bs = 0.0, bi = IDX_INVALID;
#pragma unroll
            for (uint32_t j = 0; j < TOPK_CACHE; j++) {
                const uint32_t i = lane + 64 * j;
                if (i < n && key_before(ws, wi, cs[j], i) && key_before(cs[j], i, bs, bi)) bs = cs[j], bi = i;
            }
            for (uint32_t i = lane + 64 * TOPK_CACHE; i < n; i += 64) {
                const double s = sc[i];
                if (key_before(ws, wi, s, i) && key_before(s, i, bs, bi)) bs = s, bi = i;
            }
        }
    }

    // the measure over ranks 0 .. L - 1, rank r's operands from lane r
    const bool in = lane < L;
    const uint32_t doc = base + (in ? mine : 0u);
    double result = 0.0;
    if (measure == M_DCG) {
        const double t = in ? gexp[doc] / disc[lane] : 0.0;
        for (uint32_t r = 0; r < L; r++) result = result + __shfl(t, (int)r);
    } else if (measure == M_ERR) {
        const double R = (in && gain[doc] > 0.0f) ? gexp[doc] / norm : 0.0;
        double p = 1.0;
        for (uint32_t r = 0; r < L; r++) {
            const double Rr = __shfl(R, (int)r);
            result = result + (p * Rr) / (double)(r + 1);
            p = p * (1.0 - Rr);
        }
    } else {
        const uint32_t c = (uint32_t)__popcll(__ballot(in && gain[doc] > 0.0f));
        if (measure == M_PRECISION) {
            result = (double)c / norm;
        } else if (measure == M_SUCCESS) {
            result = c != 0 ? 1.0 : 0.0;
        } else if (measure == M_RECALL) {
            uint32_t num_rel = (uint32_t)norm;
            if (count_all) {
                for (int off = 32; off > 0; off >>= 1) own_rel += __shfl_xor(own_rel, off);
                num_rel = own_rel;
            }
            if (num_rel != 0) result = (double)c / (double)num_rel;
        }
    }
    if (lane == 0) M[(size_t)q * B + b] = result;
}
