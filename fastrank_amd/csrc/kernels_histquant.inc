// Part of device.hip (single translation unit; see that file's header).  LambdaMART's quantised gradients (DESIGN.md section
// 11, "Quantised gradients"; the arithmetic and the proof of the packed layout: lambdamart_quant.hpp).  Newton gain only.
//
//   hist_quantq_kernel        (q, w) of every entry of the tree's list from its fixed-point (Q, W) under the tree's key: one
//                             u32 per full-list index, q as i16 in the high half, w as u16 in the low half.  Q / W stay, for
//                             the leaf sums.
//   hist_build_packed_kernel  hist_build_newton_kernel over the packed values: one 4-byte gather per entry, one 64-bit LDS
//                             atomic per (entry, feature) into a histogram of 8 B per bin, and on the flush the same three
//                             global atomics per touched bin into the unchanged cnt / sum / wsum arrays.

static_assert(fr::QUANT_CHUNK == HIST_CHUNK, "the packed cell's field widths are proved for HIST_CHUNK entries per workgroup");

#ifndef HIST_PACKED_FB
#define HIST_PACKED_FB 8
#endif
// features per workgroup of hist_build_packed_kernel: 8 x 256 bins x 8 B = 16 KiB of LDS at k = 256, 4 KiB at the default k = 64.
// Sixteen (-DHIST_PACKED_FB=16: 32 KiB, half the reads of idx and of the packed values) were slower: at the 30K shape with
// grad_quant_bits 4 grow_ms per tree was 3.05-3.13 ms against 2.76-2.80 ms, the kernel 0.443 ms per launch against 0.383 ms, and
// leaf-wise growth (max_leaves 32) 8.39-8.91 ms against 6.00-6.59 ms (DESIGN.md section 11, "Quantised gradients")
constexpr uint32_t HIST_FB_PACKED = HIST_PACKED_FB;
static_assert(HIST_FB_PACKED * HIST_MAX_BINS * 8u <= 64u * 1024u, "the LDS histogram fits a workgroup's 64 KiB");

// root == nullptr: the tree's list is the whole instance list.  pos / perm: the entry's position and, by position, the
// document's original instance id (goss_flag_kernel's pair).  n: the tree's list's length; d / d_w: its two shifts.
__global__ __launch_bounds__(256) void hist_quantq_kernel(const long long* __restrict__ Q, const long long* __restrict__ W,
                                                          const uint32_t* __restrict__ root, const uint32_t* __restrict__ pos,
                                                          const uint32_t* __restrict__ perm, uint32_t n, unsigned long long key, int d, int d_w,
                                                          uint32_t* __restrict__ packed) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = root ? root[i] : i;  // (packed stays indexed by the full list's index, like Q / W)
    const uint32_t id = perm[pos[r]];
    packed[r] = fr::quant_pack(fr::quant_q(Q[r], key, id, d), fr::quant_w(W[r], key, id, d_w));
}

// grid (items, feature blocks of HIST_FB_PACKED).  cnt / sum / wsum: [slot][F][k]; n: the bin matrix's row length
template <bool SEL>
__global__ __launch_bounds__(256) void hist_build_packed_kernel(const HistItemDev* __restrict__ items, const uint8_t* __restrict__ xbin,
                                                                uint32_t n, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ packed,
                                                                const uint32_t* __restrict__ fsel, uint32_t F, uint32_t k,
                                                                uint32_t* __restrict__ cnt, unsigned long long* __restrict__ sum,
                                                                unsigned long long* __restrict__ wsum) {
    constexpr uint32_t FB = HIST_FB_PACKED;
    extern __shared__ unsigned long long hist_lds[];
    const HistItemDev it = items[blockIdx.x];
    const uint32_t f0 = blockIdx.y * FB, nf = min(FB, F - f0);
    for (uint32_t t = threadIdx.x; t < FB * k; t += blockDim.x) hist_lds[t] = 0ull;
    __syncthreads();
    const uint8_t* xb0 = xbin + (size_t)f0 * n;
    const uint8_t* row[FB];  // (uniform: the block's rows of the bin matrix)
#pragma unroll
    for (uint32_t u = 0; u < FB; u++) row[u] = SEL ? xbin + (size_t)fsel[f0 + min(u, nf - 1)] * n : xb0 + (size_t)u * n;
    for (uint32_t i = it.begin + threadIdx.x; i < it.end; i += blockDim.x) {
        const uint32_t r = idx[i];
        const unsigned long long add = fr::quant_cell_add(packed[r]);
        if (nf == FB) {
            uint32_t b[FB];
#pragma unroll
            for (uint32_t u = 0; u < FB; u++) b[u] = SEL ? row[u][r] : xb0[(size_t)u * n + r];
#pragma unroll
            for (uint32_t u = 0; u < FB; u++) atomicAdd(&hist_lds[u * k + b[u]], add);
        } else {
            for (uint32_t u = 0; u < nf; u++) {
                const uint32_t b = SEL ? xbin[(size_t)fsel[f0 + u] * n + r] : xb0[(size_t)u * n + r];
                atomicAdd(&hist_lds[u * k + b], add);
            }
        }
    }
    __syncthreads();
    const size_t base = ((size_t)it.slot * F + f0) * k;
    for (uint32_t t = threadIdx.x; t < nf * k; t += blockDim.x) {
        const unsigned long long v = hist_lds[t];
        if (v == 0ull) continue;  // (a touched cell's count field is 1..HIST_CHUNK)
        atomicAdd(&cnt[base + t], fr::quant_cell_count(v));
        atomicAdd(&sum[base + t], (unsigned long long)fr::quant_cell_q(v));
        atomicAdd(&wsum[base + t], (unsigned long long)fr::quant_cell_w(v));
    }
}
