// Part of device.hip (single translation unit; see that file's header).  LambdaMART's histogram grower (DESIGN.md section 11,
// "Histogram grower"): features binned once into one byte each, gradients as int64 fixed point, per-node histograms of
// (count, sum Q) per (feature, bin).  Integer sums do not depend on their order, so the histograms may be built with
// atomics -- in LDS inside a workgroup, then one 64-bit add per touched bin to global memory -- and a sibling's histogram is
// exactly parent minus child.
//
//   hist_column_kernel    a feature's f32 column over the instance list (-0.0 read as 0.0; NaN raises a flag)
//   (rocPRIM)             radix sort of that column
//   hist_distinct_kernel  number of distinct values, and the first HIST_MAX_BINS + 1 of them (in no particular order)
//   hist_edges_kernel     the feature's at most k - 1 edges: every distinct value but the largest when there are at most k,
//                         else sorted[(j n + k - 1) / k - 1], j = 1..k-1, duplicates and the maximum dropped
//   hist_bin_kernel       bin(x) = number of edges strictly below x, so bins 0..j hold exactly x <= edge_j
//   hist_qflag_kernel / (rocPRIM exclusive scan) / hist_rootlist_kernel
//                         a tree's query sample: the ascending list of the instance-list indices whose query is flagged
//   hist_absmax_kernel    max |lambda|, max |w| over the tree's instance list (bit patterns of non-negative doubles order like them)
//   hist_quant_kernel     Q = (int64) rint(ldexp(lambda, S)), W likewise
//   hist_build_kernel     one workgroup per (stretch of a node's index list, block of HIST_FB features)
//   hist_sub_kernel       sibling = parent - child
//   hist_scan_kernel      one wave per (node, feature): prefix sums over the bins, every edge a candidate, the last maximum wins
//   hist_flag_kernel / (rocPRIM exclusive scan) / hist_scatter_kernel / hist_copy_kernel
//                         stable partition of every splitting node's stretch of the index list
//   hist_leafsum_kernel   sum Q, sum W of every leaf's stretch
// A tree's feature sample is a table fsel[F_t] of rows of the bin matrix: histograms are [slot][F_t][k] then (nullptr: all rows).

constexpr uint32_t HIST_MAX_BINS = 256;  // bins are one byte
constexpr uint32_t HIST_FB = 8;          // features per workgroup of hist_build_kernel: 8 x 256 bins x 12 B = 24 KiB of LDS, six workgroups per CU
constexpr uint32_t HIST_CHUNK = 8192;    // index-list entries per workgroup

struct HistItemDev {
    uint32_t slot, begin, end;
};
struct HistSplitDev {
    uint32_t begin, end, fslot, edge, nl;
};
struct HistSubDev {
    uint32_t parent, small, large;
};
struct HistBestDev {
    double imp;
    long long ql, qtot;
    uint32_t edge, nl, valid, pad;
};

__global__ __launch_bounds__(256) void hist_column_kernel(const float* __restrict__ xb, uint32_t dq, const uint32_t* __restrict__ pos,
                                                          uint32_t n, uint32_t f, float* __restrict__ out, int* __restrict__ nan_flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = xb[xb_index(pos[i], f, dq)] + 0.0f;
    if (v != v) atomicOr(nan_flag, 1);
    out[i] = v;
}

__global__ __launch_bounds__(256) void hist_distinct_kernel(const float* __restrict__ sorted, uint32_t n, uint32_t* __restrict__ count,
                                                            float* __restrict__ firsts /*[HIST_MAX_BINS + 1]*/) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == 0 || sorted[i] != sorted[i - 1]) {
        const uint32_t s = atomicAdd(count, 1u);
        if (s <= HIST_MAX_BINS) firsts[s] = sorted[i];
    }
}

__global__ __launch_bounds__(256) void hist_edges_kernel(const float* __restrict__ sorted, uint32_t n, uint32_t k,
                                                         const uint32_t* __restrict__ count, const float* __restrict__ firsts,
                                                         float* __restrict__ edges /*[HIST_MAX_BINS]*/, uint32_t* __restrict__ nedges) {
    __shared__ float vals[HIST_MAX_BINS + 1];
    __shared__ uint32_t keep[HIST_MAX_BINS + 1];
    const uint32_t t = threadIdx.x;
    const uint32_t nd = *count;
    if (nd <= k) {  // few distinct values: each its own bin (rank by counting: firsts[] arrives in no order)
        for (uint32_t u = t; u < nd; u += blockDim.x) vals[u] = firsts[u];
        __syncthreads();
        for (uint32_t u = t; u < nd; u += blockDim.x) {
            uint32_t r = 0;
            for (uint32_t w = 0; w < nd; w++) r += vals[w] < vals[u] ? 1u : 0u;
            if (r + 1 < nd) edges[r] = vals[u];
        }
        if (t == 0) *nedges = nd ? nd - 1 : 0;
        return;
    }
    const float vmax = sorted[n - 1];
    for (uint32_t j = t; j <= HIST_MAX_BINS; j += blockDim.x) {
        keep[j] = 0;
        if (j >= 1 && j < k) {
            const float v = sorted[((uint64_t)j * n + k - 1) / k - 1];
            vals[j] = v;
            const bool dup = j > 1 && v == sorted[((uint64_t)(j - 1) * n + k - 1) / k - 1];
            keep[j] = (!dup && v != vmax) ? 1u : 0u;
        }
    }
    __syncthreads();
    for (uint32_t j = t; j < k; j += blockDim.x) {
        if (j < 1 || !keep[j]) continue;
        uint32_t r = 0;
        for (uint32_t w = 1; w < j; w++) r += keep[w];
        edges[r] = vals[j];
    }
    if (t == 0) {
        uint32_t r = 0;
        for (uint32_t w = 1; w < k; w++) r += keep[w];
        *nedges = r;
    }
}

__global__ __launch_bounds__(256) void hist_bin_kernel(const float* __restrict__ col, uint32_t n, const float* __restrict__ edges,
                                                       const uint32_t* __restrict__ nedges, uint8_t* __restrict__ out) {
    __shared__ float e[HIST_MAX_BINS];
    const uint32_t ne = min(*nedges, HIST_MAX_BINS - 1);
    for (uint32_t u = threadIdx.x; u < ne; u += blockDim.x) e[u] = edges[u];
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = col[i];
    uint32_t lo = 0, hi = ne;  // first edge that is not below x
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (e[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    out[i] = (uint8_t)lo;
}

// flag[i] = 1 when the query of instance-list entry i is in the tree's sample (qof[i] < nq by construction)
__global__ __launch_bounds__(256) void hist_qflag_kernel(const uint32_t* __restrict__ qof, const uint8_t* __restrict__ qflag, uint32_t n,
                                                         uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = qflag[qof[i]] ? 1u : 0u;
}

// scan = exclusive prefix sums of flag: root[scan[i]] = i for every flagged i (nt: the length the host expects)
__global__ __launch_bounds__(256) void hist_rootlist_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ scan, uint32_t n,
                                                            uint32_t nt, uint32_t* __restrict__ root, uint32_t* __restrict__ total) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flag[i] && scan[i] < nt) root[scan[i]] = i;
    if (i == n - 1) *total = scan[i] + flag[i];
}

// root == nullptr: the tree's instance list is the whole one; pos == nullptr: lam / wt are already in instance-list order
__global__ __launch_bounds__(256) void hist_absmax_kernel(const double* __restrict__ lam, const double* __restrict__ wt,
                                                          const uint32_t* __restrict__ pos, const uint32_t* __restrict__ root, uint32_t n,
                                                          unsigned long long* __restrict__ out /*[2]*/) {
    unsigned long long ml = 0, mw = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t r = root ? root[i] : i;
        const uint32_t p = pos ? pos[r] : r;
        ml = max(ml, (unsigned long long)__double_as_longlong(fabs(lam[p])));
        mw = max(mw, (unsigned long long)__double_as_longlong(fabs(wt[p])));
    }
    for (int o = 32; o > 0; o >>= 1) {
        ml = max(ml, (unsigned long long)__shfl_xor((long long)ml, o));
        mw = max(mw, (unsigned long long)__shfl_xor((long long)mw, o));
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicMax(&out[0], ml);
        atomicMax(&out[1], mw);
    }
}

__global__ __launch_bounds__(256) void hist_quant_kernel(const double* __restrict__ lam, const double* __restrict__ wt,
                                                         const uint32_t* __restrict__ pos, const uint32_t* __restrict__ root, uint32_t n,
                                                         int s_l, int s_w, int w_zero, long long* __restrict__ Q,
                                                         long long* __restrict__ W) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = root ? root[i] : i;  // Q / W stay indexed by the full list's index: the build kernel reads Q[idx[i]]
    const uint32_t p = pos ? pos[r] : r;
    Q[r] = (long long)rint(ldexp(lam[p], s_l));
    W[r] = w_zero ? 0ll : (long long)rint(ldexp(wt[p], s_w));
}

__global__ __launch_bounds__(256) void hist_iota_kernel(uint32_t* __restrict__ idx, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = i;
}

// grid (items, feature blocks).  cnt / sum: [slot][F][k]; n: the bin matrix's row length.  SEL: feature u of the F is row
// fsel[u] of the bin matrix (a tree's feature sample), else row u
template <bool SEL>
__global__ __launch_bounds__(256) void hist_build_kernel(const HistItemDev* __restrict__ items, const uint8_t* __restrict__ xbin,
                                                         uint32_t n, const uint32_t* __restrict__ idx, const long long* __restrict__ Q,
                                                         const uint32_t* __restrict__ fsel, uint32_t F, uint32_t k,
                                                         uint32_t* __restrict__ cnt, unsigned long long* __restrict__ sum) {
    extern __shared__ unsigned long long hist_lds[];
    const HistItemDev it = items[blockIdx.x];
    const uint32_t f0 = blockIdx.y * HIST_FB, nf = min(HIST_FB, F - f0);
    unsigned long long* lq = hist_lds;
    uint32_t* lc = (uint32_t*)(hist_lds + (size_t)HIST_FB * k);
    for (uint32_t t = threadIdx.x; t < HIST_FB * k; t += blockDim.x) {
        lq[t] = 0ull;
        lc[t] = 0u;
    }
    __syncthreads();
    const uint8_t* xb0 = xbin + (size_t)f0 * n;
    const uint8_t* row[HIST_FB];  // (uniform: the block's rows of the bin matrix)
#pragma unroll
    for (uint32_t u = 0; u < HIST_FB; u++) row[u] = SEL ? xbin + (size_t)fsel[f0 + min(u, nf - 1)] * n : xb0 + (size_t)u * n;
    for (uint32_t i = it.begin + threadIdx.x; i < it.end; i += blockDim.x) {
        const uint32_t r = idx[i];
        const unsigned long long q = (unsigned long long)Q[r];
        if (nf == HIST_FB) {
            uint32_t b[HIST_FB];
#pragma unroll
            for (uint32_t u = 0; u < HIST_FB; u++) b[u] = SEL ? row[u][r] : xb0[(size_t)u * n + r];
#pragma unroll
            for (uint32_t u = 0; u < HIST_FB; u++) {
                atomicAdd(&lq[u * k + b[u]], q);
                atomicAdd(&lc[u * k + b[u]], 1u);
            }
        } else {
            for (uint32_t u = 0; u < nf; u++) {
                const uint32_t b = SEL ? xbin[(size_t)fsel[f0 + u] * n + r] : xb0[(size_t)u * n + r];
                atomicAdd(&lq[u * k + b], q);
                atomicAdd(&lc[u * k + b], 1u);
            }
        }
    }
    __syncthreads();
    const size_t base = ((size_t)it.slot * F + f0) * k;
    for (uint32_t t = threadIdx.x; t < nf * k; t += blockDim.x) {
        const uint32_t c = lc[t];
        if (c == 0) continue;
        atomicAdd(&cnt[base + t], c);
        atomicAdd(&sum[base + t], lq[t]);
    }
}

// grid (pairs, ceil(F k / 256)): the larger child's histogram = the parent's (previous level) - the smaller child's
__global__ __launch_bounds__(256) void hist_sub_kernel(const HistSubDev* __restrict__ pairs, uint32_t fk, const uint32_t* __restrict__ pcnt,
                                                       const unsigned long long* __restrict__ psum, uint32_t* __restrict__ cnt,
                                                       unsigned long long* __restrict__ sum) {
    const HistSubDev pr = pairs[blockIdx.x];
    const uint32_t t = blockIdx.y * blockDim.x + threadIdx.x;
    if (t >= fk) return;
    const size_t p = (size_t)pr.parent * fk + t, s = (size_t)pr.small * fk + t, l = (size_t)pr.large * fk + t;
    cnt[l] = pcnt[p] - cnt[s];
    sum[l] = psum[p] - sum[s];
}

// one wave per (node, feature); nodes[a] = {slot, begin, end} of the a-th open node; best[a * F + f]; fsel: as above
__global__ __launch_bounds__(64) void hist_scan_kernel(const HistItemDev* __restrict__ nodes, uint32_t F, uint32_t k,
                                                       const uint32_t* __restrict__ nedges, const uint32_t* __restrict__ fsel,
                                                       const uint32_t* __restrict__ cnt,
                                                       const unsigned long long* __restrict__ sum, uint32_t min_leaf,
                                                       HistBestDev* __restrict__ best) {
    const uint32_t a = blockIdx.x / F, f = blockIdx.x % F, lane = threadIdx.x;
    const HistItemDev nd = nodes[a];
    const uint32_t n = nd.end - nd.begin;
    const uint32_t ne = min(nedges[fsel ? fsel[f] : f], k - 1);
    const size_t base = ((size_t)nd.slot * F + f) * k;
    const uint32_t B = (k + 63) / 64;  // bins per lane (<= 4)
    uint32_t c[4];
    long long s[4];
    uint32_t tc = 0;
    long long ts = 0;
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t b = lane * B + u;
        const bool in = u < B && b < k;
        c[u] = in ? cnt[base + b] : 0u;
        s[u] = in ? (long long)sum[base + b] : 0ll;
        tc += c[u];
        ts += s[u];
    }
    uint32_t ic = tc;
    long long is = ts;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t oc = __shfl_up(ic, o);
        const long long os = __shfl_up(is, o);
        if ((int)lane >= o) {
            ic += oc;
            is += os;
        }
    }
    const long long qtot = __shfl(is, 63);
    uint32_t rc = ic - tc;  // counts / sums of the bins before this lane's
    long long rs = is - ts;
    double bimp = 0.0;
    uint32_t bj = 0, bnl = 0, have = 0;
    long long bql = 0;
    for (uint32_t u = 0; u < B; u++) {
        const uint32_t j = lane * B + u;
        rc += c[u];
        rs += s[u];
        if (j >= ne) break;
        const uint32_t nl = rc, nr = n - rc;
        if (nl == 0 || nr == 0 || nl < min_leaf || nr < min_leaf) continue;
        const double sl = (double)rs, sr = (double)(qtot - rs);
        const double imp = (sl * sl) / (double)nl + (sr * sr) / (double)nr;
        if (!have || imp >= bimp) {
            have = 1;
            bimp = imp;
            bj = j;
            bnl = nl;
            bql = rs;
        }
    }
    // the last maximum over the lanes: larger importance, then the later edge
    double wimp = bimp;
    uint32_t wj = bj, whave = have;
    for (int o = 32; o > 0; o >>= 1) {
        const double oimp = __shfl_xor(wimp, o);
        const uint32_t oj = __shfl_xor(wj, o), ohave = __shfl_xor(whave, o);
        if (ohave && (!whave || oimp > wimp || (oimp == wimp && oj > wj))) {
            whave = 1;
            wimp = oimp;
            wj = oj;
        }
    }
    HistBestDev* out = best + (size_t)a * F + f;
    if (!whave) {
        if (lane == 0) *out = HistBestDev{0.0, 0ll, qtot, 0u, 0u, 0u, 0u};
    } else if (have && bj == wj) {
        *out = HistBestDev{bimp, bql, qtot, bj, bnl, 1u, 0u};
    }
}

// grid: chunks of the splitting nodes' stretches.  items[i].slot = index into splits
__global__ __launch_bounds__(256) void hist_flag_kernel(const HistItemDev* __restrict__ items, const HistSplitDev* __restrict__ splits,
                                                        const uint8_t* __restrict__ xbin, uint32_t n, const uint32_t* __restrict__ idx,
                                                        uint32_t* __restrict__ flag) {
    const HistItemDev it = items[blockIdx.x];
    const HistSplitDev sp = splits[it.slot];
    const uint8_t* col = xbin + (size_t)sp.fslot * n;
    for (uint32_t i = it.begin + threadIdx.x; i < it.end; i += blockDim.x) flag[i] = col[idx[i]] <= sp.edge ? 1u : 0u;
}

// scan = exclusive prefix sums of flag over the whole list; inside a node only differences are used
__global__ __launch_bounds__(256) void hist_scatter_kernel(const HistItemDev* __restrict__ items, const HistSplitDev* __restrict__ splits,
                                                           const uint32_t* __restrict__ flag, const uint32_t* __restrict__ scan,
                                                           const uint32_t* __restrict__ idx, uint32_t* __restrict__ out) {
    const HistItemDev it = items[blockIdx.x];
    const HistSplitDev sp = splits[it.slot];
    const uint32_t s0 = scan[sp.begin];
    for (uint32_t i = it.begin + threadIdx.x; i < it.end; i += blockDim.x) {
        const uint32_t lb = scan[i] - s0;  // left-goers before i in the node
        const uint32_t d = flag[i] ? sp.begin + lb : sp.begin + sp.nl + (i - sp.begin - lb);
        if (d < sp.end) out[d] = idx[i];
    }
}

__global__ __launch_bounds__(256) void hist_copy_kernel(const HistItemDev* __restrict__ items, const uint32_t* __restrict__ src,
                                                        uint32_t* __restrict__ dst) {
    const HistItemDev it = items[blockIdx.x];
    for (uint32_t i = it.begin + threadIdx.x; i < it.end; i += blockDim.x) dst[i] = src[i];
}

// items[i].slot = leaf number; out[leaf * 2] += sum Q, out[leaf * 2 + 1] += sum W
__global__ __launch_bounds__(256) void hist_leafsum_kernel(const HistItemDev* __restrict__ items, const uint32_t* __restrict__ idx,
                                                           const long long* __restrict__ Q, const long long* __restrict__ W,
                                                           unsigned long long* __restrict__ out) {
    const HistItemDev it = items[blockIdx.x];
    long long q = 0, w = 0;
    for (uint32_t i = it.begin + threadIdx.x; i < it.end; i += blockDim.x) {
        const uint32_t r = idx[i];
        q += Q[r];
        w += W[r];
    }
    for (int o = 32; o > 0; o >>= 1) {
        q += __shfl_xor(q, o);
        w += __shfl_xor(w, o);
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(&out[(size_t)it.slot * 2], (unsigned long long)q);
        atomicAdd(&out[(size_t)it.slot * 2 + 1], (unsigned long long)w);
    }
}

// --- Newton split gain (DESIGN.md section 11, "Newton split gain") -------------------------------------------------------
// The histograms carry a third quantity, sum W per (feature, bin): [slot][F][k] of (count u32, sum Q i64, sum W i64), 20 B
// per bin.  The kernels above keep their code; these stand next to them and run only for split_gain = "newton".
//
//   hist_build_newton_kernel  hist_build_kernel with a third LDS atomic per (entry, feature) and a third global one per touched bin
//   hist_sub_newton_kernel    sibling = parent - child, three arrays
//   hist_scan_newton_kernel   three prefix sums; G = ldexp(Q, -S), H = ldexp(W, -S_w), term = (G G) / (H + lambda_l2);
//                             a candidate also needs H >= min_sum_hessian and H + lambda_l2 > 0 on both sides

#ifndef HIST_NEWTON_FB
#define HIST_NEWTON_FB 8
#endif
// features per workgroup of hist_build_newton_kernel: 8 x 256 bins x 20 B = 40 KiB of LDS at k = 256 (four workgroups per CU
// of 160 KiB, against six of hist_build_kernel), 10 KiB at the default k = 64.  Four features per workgroup (-DHIST_NEWTON_FB=4)
// halve the footprint but read idx, Q and W twice as often: at the 30K shape grow_ms per tree was 5.06-5.17 ms against
// 4.68-4.81 ms (6-10 % more), 100 trees 1.183-1.193 s against 1.144-1.197 s (DESIGN.md section 11, "Newton split gain")
constexpr uint32_t HIST_FB_NEWTON = HIST_NEWTON_FB;

struct HistBestNewtonDev {
    double imp;
    long long ql, qtot, wl, wtot;
    uint32_t edge, nl, valid, pad;
};

// grid (items, feature blocks of HIST_FB_NEWTON).  cnt / sum / wsum: [slot][F][k]
template <bool SEL>
__global__ __launch_bounds__(256) void hist_build_newton_kernel(const HistItemDev* __restrict__ items, const uint8_t* __restrict__ xbin,
                                                                uint32_t n, const uint32_t* __restrict__ idx, const long long* __restrict__ Q,
                                                                const long long* __restrict__ W, const uint32_t* __restrict__ fsel, uint32_t F,
                                                                uint32_t k, uint32_t* __restrict__ cnt, unsigned long long* __restrict__ sum,
                                                                unsigned long long* __restrict__ wsum) {
    constexpr uint32_t FB = HIST_FB_NEWTON;
    extern __shared__ unsigned long long hist_lds[];
    const HistItemDev it = items[blockIdx.x];
    const uint32_t f0 = blockIdx.y * FB, nf = min(FB, F - f0);
    unsigned long long* lq = hist_lds;
    unsigned long long* lw = hist_lds + (size_t)FB * k;
    uint32_t* lc = (uint32_t*)(hist_lds + (size_t)2 * FB * k);
    for (uint32_t t = threadIdx.x; t < FB * k; t += blockDim.x) {
        lq[t] = 0ull;
        lw[t] = 0ull;
        lc[t] = 0u;
    }
    __syncthreads();
    const uint8_t* xb0 = xbin + (size_t)f0 * n;
    const uint8_t* row[FB];  // (uniform: the block's rows of the bin matrix)
#pragma unroll
    for (uint32_t u = 0; u < FB; u++) row[u] = SEL ? xbin + (size_t)fsel[f0 + min(u, nf - 1)] * n : xb0 + (size_t)u * n;
    for (uint32_t i = it.begin + threadIdx.x; i < it.end; i += blockDim.x) {
        const uint32_t r = idx[i];
        const unsigned long long q = (unsigned long long)Q[r], w = (unsigned long long)W[r];
        if (nf == FB) {
            uint32_t b[FB];
#pragma unroll
            for (uint32_t u = 0; u < FB; u++) b[u] = SEL ? row[u][r] : xb0[(size_t)u * n + r];
#pragma unroll
            for (uint32_t u = 0; u < FB; u++) {
                atomicAdd(&lq[u * k + b[u]], q);
                atomicAdd(&lw[u * k + b[u]], w);
                atomicAdd(&lc[u * k + b[u]], 1u);
            }
        } else {
            for (uint32_t u = 0; u < nf; u++) {
                const uint32_t b = SEL ? xbin[(size_t)fsel[f0 + u] * n + r] : xb0[(size_t)u * n + r];
                atomicAdd(&lq[u * k + b], q);
                atomicAdd(&lw[u * k + b], w);
                atomicAdd(&lc[u * k + b], 1u);
            }
        }
    }
    __syncthreads();
    const size_t base = ((size_t)it.slot * F + f0) * k;
    for (uint32_t t = threadIdx.x; t < nf * k; t += blockDim.x) {
        const uint32_t c = lc[t];
        if (c == 0) continue;
        atomicAdd(&cnt[base + t], c);
        atomicAdd(&sum[base + t], lq[t]);
        atomicAdd(&wsum[base + t], lw[t]);
    }
}

// grid (pairs, ceil(F k / 256))
__global__ __launch_bounds__(256) void hist_sub_newton_kernel(const HistSubDev* __restrict__ pairs, uint32_t fk, const uint32_t* __restrict__ pcnt,
                                                              const unsigned long long* __restrict__ psum,
                                                              const unsigned long long* __restrict__ pwsum, uint32_t* __restrict__ cnt,
                                                              unsigned long long* __restrict__ sum, unsigned long long* __restrict__ wsum) {
    const HistSubDev pr = pairs[blockIdx.x];
    const uint32_t t = blockIdx.y * blockDim.x + threadIdx.x;
    if (t >= fk) return;
    const size_t p = (size_t)pr.parent * fk + t, s = (size_t)pr.small * fk + t, l = (size_t)pr.large * fk + t;
    cnt[l] = pcnt[p] - cnt[s];
    sum[l] = psum[p] - sum[s];
    wsum[l] = pwsum[p] - wsum[s];
}

// (G G) / (H + lambda_l2) of the integer pair (q, w); every operation rounded on its own
__device__ __forceinline__ double hist_newton_term(long long q, double h, int s_l, double l2) {
    const double g = ldexp((double)q, -s_l);
    return (g * g) / (h + l2);
}

// one wave per (node, feature), as hist_scan_kernel
__global__ __launch_bounds__(64) void hist_scan_newton_kernel(const HistItemDev* __restrict__ nodes, uint32_t F, uint32_t k,
                                                              const uint32_t* __restrict__ nedges, const uint32_t* __restrict__ fsel,
                                                              const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ sum,
                                                              const unsigned long long* __restrict__ wsum, uint32_t min_leaf, int s_l, int s_w,
                                                              double l2, double min_hess, HistBestNewtonDev* __restrict__ best) {
    const uint32_t a = blockIdx.x / F, f = blockIdx.x % F, lane = threadIdx.x;
    const HistItemDev nd = nodes[a];
    const uint32_t n = nd.end - nd.begin;
    const uint32_t ne = min(nedges[fsel ? fsel[f] : f], k - 1);
    const size_t base = ((size_t)nd.slot * F + f) * k;
    const uint32_t B = (k + 63) / 64;  // bins per lane (<= 4)
    uint32_t c[4];
    long long s[4], w[4];
    uint32_t tc = 0;
    long long ts = 0, tw = 0;
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t b = lane * B + u;
        const bool in = u < B && b < k;
        c[u] = in ? cnt[base + b] : 0u;
        s[u] = in ? (long long)sum[base + b] : 0ll;
        w[u] = in ? (long long)wsum[base + b] : 0ll;
        tc += c[u];
        ts += s[u];
        tw += w[u];
    }
    uint32_t ic = tc;
    long long is = ts, iw = tw;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t oc = __shfl_up(ic, o);
        const long long os = __shfl_up(is, o), ow = __shfl_up(iw, o);
        if ((int)lane >= o) {
            ic += oc;
            is += os;
            iw += ow;
        }
    }
    const long long qtot = __shfl(is, 63), wtot = __shfl(iw, 63);
    uint32_t rc = ic - tc;  // counts / sums of the bins before this lane's
    long long rs = is - ts, rw = iw - tw;
    double bimp = 0.0;
    uint32_t bj = 0, bnl = 0, have = 0;
    long long bql = 0, bwl = 0;
    for (uint32_t u = 0; u < B; u++) {
        const uint32_t j = lane * B + u;
        rc += c[u];
        rs += s[u];
        rw += w[u];
        if (j >= ne) break;
        const uint32_t nl = rc, nr = n - rc;
        if (nl == 0 || nr == 0 || nl < min_leaf || nr < min_leaf) continue;
        const double hl = ldexp((double)rw, -s_w), hr = ldexp((double)(wtot - rw), -s_w);
        if (!(hl >= min_hess && hr >= min_hess && hl + l2 > 0.0 && hr + l2 > 0.0)) continue;
        const double imp = hist_newton_term(rs, hl, s_l, l2) + hist_newton_term(qtot - rs, hr, s_l, l2);
        if (!have || imp >= bimp) {
            have = 1;
            bimp = imp;
            bj = j;
            bnl = nl;
            bql = rs;
            bwl = rw;
        }
    }
    // the last maximum over the lanes: larger importance, then the later edge
    double wimp = bimp;
    uint32_t wj = bj, whave = have;
    for (int o = 32; o > 0; o >>= 1) {
        const double oimp = __shfl_xor(wimp, o);
        const uint32_t oj = __shfl_xor(wj, o), ohave = __shfl_xor(whave, o);
        if (ohave && (!whave || oimp > wimp || (oimp == wimp && oj > wj))) {
            whave = 1;
            wimp = oimp;
            wj = oj;
        }
    }
    HistBestNewtonDev* out = best + (size_t)a * F + f;
    if (!whave) {
        if (lane == 0) *out = HistBestNewtonDev{0.0, 0ll, qtot, 0ll, wtot, 0u, 0u, 0u, 0u};
    } else if (have && bj == wj) {
        *out = HistBestNewtonDev{bimp, bql, qtot, bwl, wtot, bj, bnl, 1u, 0u};
    }
}

// --- Leaf-wise growth (DESIGN.md section 11, "Leaf-wise growth") ---------------------------------------------------------
// max_leaves >= 2: one leaf is split at a time, the open leaf with the largest gain.  The histograms live in a pool of slots
// [slot][F][k] (the same three arrays; wsum only under the Newton gain); the larger child takes over its parent's slot, the
// subtraction happens in place.  One split step works on one stretch, so the stretch and the slots are kernel arguments and
// no table is uploaded but the build kernel's items.  The kernels above keep their code; these run only for max_leaves >= 2.
//
//   hist_leaf_flag_kernel / (rocPRIM exclusive scan of the stretch) / hist_leaf_scatter_kernel
//                           stable partition of the one stretch [begin, end)
//   hist_leaf_scan_kernel   one wave per (child, feature): a child marked `derive` is first made in place, parent - sibling,
//                           then scanned; the arithmetic of a candidate is hist_scan_kernel's / hist_scan_newton_kernel's
//   hist_pick_kernel        one wave per child: its F per-feature records reduced to the node's single one, the last maximum
//                           over the tree's feature order, and the winning feature's index among the F

struct HistPickDev {
    double imp;
    long long ql, qtot, wl, wtot;  // (wl, wtot: 0 under the variance criterion)
    uint32_t edge, nl, valid, fi;  // fi: the winning feature's index among the tree's F
};
// the (at most two) children a step scans: derive != 0: slot (the parent's) becomes parent - slot `other` first
struct HistLeafKids {
    uint32_t slot[2], n[2], derive[2], other[2];
};

__global__ __launch_bounds__(256) void hist_leaf_flag_kernel(uint32_t begin, uint32_t end, const uint8_t* __restrict__ col, uint32_t edge,
                                                             const uint32_t* __restrict__ idx, uint32_t* __restrict__ flag) {
    const uint32_t i = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < end) flag[i] = col[idx[i]] <= edge ? 1u : 0u;
}

// scan[begin..end) = exclusive prefix sums of flag[begin..end) (0 at begin)
__global__ __launch_bounds__(256) void hist_leaf_scatter_kernel(uint32_t begin, uint32_t end, uint32_t nl, const uint32_t* __restrict__ flag,
                                                                const uint32_t* __restrict__ scan, const uint32_t* __restrict__ idx,
                                                                uint32_t* __restrict__ out) {
    const uint32_t i = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= end) return;
    const uint32_t lb = scan[i];  // left-goers before i in the node
    const uint32_t d = flag[i] ? begin + lb : begin + nl + (i - begin - lb);
    if (d < end) out[d] = idx[i];
}

// grid (F, children).  rec[child * F + f]
template <bool NEWTON>
__global__ __launch_bounds__(64) void hist_leaf_scan_kernel(HistLeafKids kids, uint32_t F, uint32_t k, const uint32_t* __restrict__ nedges,
                                                            const uint32_t* __restrict__ fsel, uint32_t* cnt, unsigned long long* sum,
                                                            unsigned long long* wsum, uint32_t min_leaf, int s_l, int s_w, double l2,
                                                            double min_hess, HistPickDev* __restrict__ rec) {
    const uint32_t f = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const uint32_t n = kids.n[a];
    const uint32_t ne = min(nedges[fsel ? fsel[f] : f], k - 1);
    const size_t base = ((size_t)kids.slot[a] * F + f) * k, obase = ((size_t)kids.other[a] * F + f) * k;
    const bool derive = kids.derive[a] != 0;
    const uint32_t B = (k + 63) / 64;  // bins per lane (<= 4)
    uint32_t c[4];
    long long s[4], w[4];
    uint32_t tc = 0;
    long long ts = 0, tw = 0;
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t b = lane * B + u;
        const bool in = u < B && b < k;
        c[u] = in ? cnt[base + b] : 0u;
        s[u] = in ? (long long)sum[base + b] : 0ll;
        w[u] = NEWTON && in ? (long long)wsum[base + b] : 0ll;
        if (derive && in) {  // (this wave alone reads and writes the bins of (slot, f))
            c[u] -= cnt[obase + b];
            s[u] -= (long long)sum[obase + b];
            cnt[base + b] = c[u];
            sum[base + b] = (unsigned long long)s[u];
            if (NEWTON) {
                w[u] -= (long long)wsum[obase + b];
                wsum[base + b] = (unsigned long long)w[u];
            }
        }
        tc += c[u];
        ts += s[u];
        tw += w[u];
    }
    uint32_t ic = tc;
    long long is = ts, iw = tw;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t oc = __shfl_up(ic, o);
        const long long os = __shfl_up(is, o), ow = __shfl_up(iw, o);
        if ((int)lane >= o) {
            ic += oc;
            is += os;
            iw += ow;
        }
    }
    const long long qtot = __shfl(is, 63), wtot = __shfl(iw, 63);
    uint32_t rc = ic - tc;  // counts / sums of the bins before this lane's
    long long rs = is - ts, rw = iw - tw;
    double bimp = 0.0;
    uint32_t bj = 0, bnl = 0, have = 0;
    long long bql = 0, bwl = 0;
    for (uint32_t u = 0; u < B; u++) {
        const uint32_t j = lane * B + u;
        rc += c[u];
        rs += s[u];
        rw += w[u];
        if (j >= ne) break;
        const uint32_t nl = rc, nr = n - rc;
        if (nl == 0 || nr == 0 || nl < min_leaf || nr < min_leaf) continue;
        double imp;
        if (NEWTON) {
            const double hl = ldexp((double)rw, -s_w), hr = ldexp((double)(wtot - rw), -s_w);
            if (!(hl >= min_hess && hr >= min_hess && hl + l2 > 0.0 && hr + l2 > 0.0)) continue;
            imp = hist_newton_term(rs, hl, s_l, l2) + hist_newton_term(qtot - rs, hr, s_l, l2);
        } else {
            const double sl = (double)rs, sr = (double)(qtot - rs);
            imp = (sl * sl) / (double)nl + (sr * sr) / (double)nr;
        }
        if (!have || imp >= bimp) {
            have = 1;
            bimp = imp;
            bj = j;
            bnl = nl;
            bql = rs;
            bwl = rw;
        }
    }
    // the last maximum over the lanes: larger importance, then the later edge
    double wimp = bimp;
    uint32_t wj = bj, whave = have;
    for (int o = 32; o > 0; o >>= 1) {
        const double oimp = __shfl_xor(wimp, o);
        const uint32_t oj = __shfl_xor(wj, o), ohave = __shfl_xor(whave, o);
        if (ohave && (!whave || oimp > wimp || (oimp == wimp && oj > wj))) {
            whave = 1;
            wimp = oimp;
            wj = oj;
        }
    }
    HistPickDev* out = rec + (size_t)a * F + f;
    if (!whave) {
        if (lane == 0) *out = HistPickDev{0.0, 0ll, qtot, 0ll, wtot, 0u, 0u, 0u, f};
    } else if (have && bj == wj) {
        *out = HistPickDev{bimp, bql, qtot, bwl, wtot, bj, bnl, 1u, f};
    }
}

// grid (children).  pick[a] = the last maximum of rec[a * F .. a * F + F): larger importance, then the later feature; a node
// without a valid record keeps valid = 0 and its totals
__global__ __launch_bounds__(64) void hist_pick_kernel(const HistPickDev* __restrict__ rec, uint32_t F, HistPickDev* __restrict__ pick) {
    const uint32_t a = blockIdx.x, lane = threadIdx.x;
    const HistPickDev* r = rec + (size_t)a * F;
    double wimp = 0.0;
    uint32_t wf = 0, whave = 0;
    for (uint32_t f = lane; f < F; f += 64) {  // ascending: >= keeps the later one
        if (r[f].valid && (!whave || r[f].imp >= wimp)) whave = 1, wimp = r[f].imp, wf = f;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double oimp = __shfl_xor(wimp, o);
        const uint32_t of = __shfl_xor(wf, o), ohave = __shfl_xor(whave, o);
        if (ohave && (!whave || oimp > wimp || (oimp == wimp && of > wf))) {
            whave = 1;
            wimp = oimp;
            wf = of;
        }
    }
    if (lane == 0) pick[a] = r[whave ? wf : 0];
}

// --- Monotone constraints (DESIGN.md section 11, "Monotone constraints") --------------------------------------------------
// Some feature carries a sign c in {-1, 0, +1} (sign[] by row of the bin matrix, indexed like nedges) and every node an
// interval [lo, hi] of f64 for its output.  A side's output G / (H + lambda_l2) is clamped to the interval; a side that was
// not clamped keeps the Newton term bit for bit, a clamped one has (2 G) v - ((H + lambda_l2) v) v; a candidate on a feature
// with c = +1 also needs vL <= vR, with c = -1 vL >= vR.  The records are the Newton kernels' (the host derives vL, vR and
// the children's intervals again from ql, qtot, wl, wtot).  The kernels above keep their code; these stand next to them and
// run only when some sign is not 0.
//
//   hist_scan_monotone_kernel       hist_scan_newton_kernel with bounds[node] and sign[feature]
//   hist_leaf_scan_monotone_kernel  hist_leaf_scan_kernel<true> with one interval per child

struct HistBoundsDev {
    double lo, hi;
};
// the intervals of the (at most two) children a leaf-wise step scans
struct HistLeafBoundsDev {
    double lo[2], hi[2];
};

// term of one side of a candidate (h + l2 > 0) under [lo, hi]; *v: its clamped output.  Both terms are computed and one is
// selected: the lanes of a wave disagree about which one they need
__device__ __forceinline__ double hist_monotone_term(long long q, double h, int s_l, double l2, double lo, double hi, double* v) {
    const double g = ldexp((double)q, -s_l), den = h + l2;
    const double out = g / den;
    double c = out < lo ? lo : out;
    c = c > hi ? hi : c;
    const double plain = (g * g) / den;
    const double bound = (2.0 * g) * c - (den * c) * c;
    *v = c;
    return c == out ? plain : bound;
}

// (validity as hist_scan_newton_kernel's; false: no candidate)
__device__ __forceinline__ bool hist_monotone_candidate(long long ql, long long wl, long long qtot, long long wtot, int s_l, int s_w, double l2,
                                                        double min_hess, double lo, double hi, int sign, double* imp) {
    const double hl = ldexp((double)wl, -s_w), hr = ldexp((double)(wtot - wl), -s_w);
    if (!(hl >= min_hess && hr >= min_hess && hl + l2 > 0.0 && hr + l2 > 0.0)) return false;
    double vl, vr;
    const double tl = hist_monotone_term(ql, hl, s_l, l2, lo, hi, &vl), tr = hist_monotone_term(qtot - ql, hr, s_l, l2, lo, hi, &vr);
    if ((sign > 0 && !(vl <= vr)) || (sign < 0 && !(vl >= vr))) return false;
    *imp = tl + tr;
    return true;
}

// one wave per (node, feature), as hist_scan_newton_kernel.  bounds[a]: node a's interval
__global__ __launch_bounds__(64) void hist_scan_monotone_kernel(const HistItemDev* __restrict__ nodes, const HistBoundsDev* __restrict__ bounds,
                                                                uint32_t F, uint32_t k, const uint32_t* __restrict__ nedges,
                                                                const int* __restrict__ sign, const uint32_t* __restrict__ fsel,
                                                                const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ sum,
                                                                const unsigned long long* __restrict__ wsum, uint32_t min_leaf, int s_l, int s_w,
                                                                double l2, double min_hess, HistBestNewtonDev* __restrict__ best) {
    const uint32_t a = blockIdx.x / F, f = blockIdx.x % F, lane = threadIdx.x;
    const HistItemDev nd = nodes[a];
    const HistBoundsDev bd = bounds[a];
    const uint32_t n = nd.end - nd.begin;
    const uint32_t row = fsel ? fsel[f] : f;
    const uint32_t ne = min(nedges[row], k - 1);
    const int sg = sign[row];
    const size_t base = ((size_t)nd.slot * F + f) * k;
    const uint32_t B = (k + 63) / 64;  // bins per lane (<= 4)
    uint32_t c[4];
    long long s[4], w[4];
    uint32_t tc = 0;
    long long ts = 0, tw = 0;
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t b = lane * B + u;
        const bool in = u < B && b < k;
        c[u] = in ? cnt[base + b] : 0u;
        s[u] = in ? (long long)sum[base + b] : 0ll;
        w[u] = in ? (long long)wsum[base + b] : 0ll;
        tc += c[u];
        ts += s[u];
        tw += w[u];
    }
    uint32_t ic = tc;
    long long is = ts, iw = tw;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t oc = __shfl_up(ic, o);
        const long long os = __shfl_up(is, o), ow = __shfl_up(iw, o);
        if ((int)lane >= o) {
            ic += oc;
            is += os;
            iw += ow;
        }
    }
    const long long qtot = __shfl(is, 63), wtot = __shfl(iw, 63);
    uint32_t rc = ic - tc;  // counts / sums of the bins before this lane's
    long long rs = is - ts, rw = iw - tw;
    double bimp = 0.0;
    uint32_t bj = 0, bnl = 0, have = 0;
    long long bql = 0, bwl = 0;
    for (uint32_t u = 0; u < B; u++) {
        const uint32_t j = lane * B + u;
        rc += c[u];
        rs += s[u];
        rw += w[u];
        if (j >= ne) break;
        const uint32_t nl = rc, nr = n - rc;
        if (nl == 0 || nr == 0 || nl < min_leaf || nr < min_leaf) continue;
        double imp;
        if (!hist_monotone_candidate(rs, rw, qtot, wtot, s_l, s_w, l2, min_hess, bd.lo, bd.hi, sg, &imp)) continue;
        if (!have || imp >= bimp) {
            have = 1;
            bimp = imp;
            bj = j;
            bnl = nl;
            bql = rs;
            bwl = rw;
        }
    }
    // the last maximum over the lanes: larger importance, then the later edge
    double wimp = bimp;
    uint32_t wj = bj, whave = have;
    for (int o = 32; o > 0; o >>= 1) {
        const double oimp = __shfl_xor(wimp, o);
        const uint32_t oj = __shfl_xor(wj, o), ohave = __shfl_xor(whave, o);
        if (ohave && (!whave || oimp > wimp || (oimp == wimp && oj > wj))) {
            whave = 1;
            wimp = oimp;
            wj = oj;
        }
    }
    HistBestNewtonDev* out = best + (size_t)a * F + f;
    if (!whave) {
        if (lane == 0) *out = HistBestNewtonDev{0.0, 0ll, qtot, 0ll, wtot, 0u, 0u, 0u, 0u};
    } else if (have && bj == wj) {
        *out = HistBestNewtonDev{bimp, bql, qtot, bwl, wtot, bj, bnl, 1u, 0u};
    }
}

// grid (F, children), as hist_leaf_scan_kernel<true>: the in-place parent - sibling derivation, then the scan under the child's
// own interval.  rec[child * F + f]
__global__ __launch_bounds__(64) void hist_leaf_scan_monotone_kernel(HistLeafKids kids, HistLeafBoundsDev bounds, uint32_t F, uint32_t k,
                                                                     const uint32_t* __restrict__ nedges, const int* __restrict__ sign,
                                                                     const uint32_t* __restrict__ fsel, uint32_t* cnt, unsigned long long* sum,
                                                                     unsigned long long* wsum, uint32_t min_leaf, int s_l, int s_w, double l2,
                                                                     double min_hess, HistPickDev* __restrict__ rec) {
    const uint32_t f = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const uint32_t n = kids.n[a];
    const double lo = bounds.lo[a], hi = bounds.hi[a];
    const uint32_t row = fsel ? fsel[f] : f;
    const uint32_t ne = min(nedges[row], k - 1);
    const int sg = sign[row];
    const size_t base = ((size_t)kids.slot[a] * F + f) * k, obase = ((size_t)kids.other[a] * F + f) * k;
    const bool derive = kids.derive[a] != 0;
    const uint32_t B = (k + 63) / 64;  // bins per lane (<= 4)
    uint32_t c[4];
    long long s[4], w[4];
    uint32_t tc = 0;
    long long ts = 0, tw = 0;
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t b = lane * B + u;
        const bool in = u < B && b < k;
        c[u] = in ? cnt[base + b] : 0u;
        s[u] = in ? (long long)sum[base + b] : 0ll;
        w[u] = in ? (long long)wsum[base + b] : 0ll;
        if (derive && in) {  // (this wave alone reads and writes the bins of (slot, f))
            c[u] -= cnt[obase + b];
            s[u] -= (long long)sum[obase + b];
            w[u] -= (long long)wsum[obase + b];
            cnt[base + b] = c[u];
            sum[base + b] = (unsigned long long)s[u];
            wsum[base + b] = (unsigned long long)w[u];
        }
        tc += c[u];
        ts += s[u];
        tw += w[u];
    }
    uint32_t ic = tc;
    long long is = ts, iw = tw;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t oc = __shfl_up(ic, o);
        const long long os = __shfl_up(is, o), ow = __shfl_up(iw, o);
        if ((int)lane >= o) {
            ic += oc;
            is += os;
            iw += ow;
        }
    }
    const long long qtot = __shfl(is, 63), wtot = __shfl(iw, 63);
    uint32_t rc = ic - tc;  // counts / sums of the bins before this lane's
    long long rs = is - ts, rw = iw - tw;
    double bimp = 0.0;
    uint32_t bj = 0, bnl = 0, have = 0;
    long long bql = 0, bwl = 0;
    for (uint32_t u = 0; u < B; u++) {
        const uint32_t j = lane * B + u;
        rc += c[u];
        rs += s[u];
        rw += w[u];
        if (j >= ne) break;
        const uint32_t nl = rc, nr = n - rc;
        if (nl == 0 || nr == 0 || nl < min_leaf || nr < min_leaf) continue;
        double imp;
        if (!hist_monotone_candidate(rs, rw, qtot, wtot, s_l, s_w, l2, min_hess, lo, hi, sg, &imp)) continue;
        if (!have || imp >= bimp) {
            have = 1;
            bimp = imp;
            bj = j;
            bnl = nl;
            bql = rs;
            bwl = rw;
        }
    }
    // the last maximum over the lanes: larger importance, then the later edge
    double wimp = bimp;
    uint32_t wj = bj, whave = have;
    for (int o = 32; o > 0; o >>= 1) {
        const double oimp = __shfl_xor(wimp, o);
        const uint32_t oj = __shfl_xor(wj, o), ohave = __shfl_xor(whave, o);
        if (ohave && (!whave || oimp > wimp || (oimp == wimp && oj > wj))) {
            whave = 1;
            wimp = oimp;
            wj = oj;
        }
    }
    HistPickDev* out = rec + (size_t)a * F + f;
    if (!whave) {
        if (lane == 0) *out = HistPickDev{0.0, 0ll, qtot, 0ll, wtot, 0u, 0u, 0u, f};
    } else if (have && bj == wj) {
        *out = HistPickDev{bimp, bql, qtot, bwl, wtot, bj, bnl, 1u, f};
    }
}

// --- Symmetric trees (DESIGN.md section 11, "Symmetric trees") -----------------------------------------------------------
// symmetric_trees: every node of a level splits on one (feature, edge).  A candidate's level importance I(f, j) is the
// sequential f64 sum, over the level's open nodes in their order, of the node's own candidate importance where the node
// splits under (f, j) by the plain rule and of the node's unsplit term where it does not; the candidate is valid when some
// node splits under it; the last maximum of I over the valid candidates wins (a NaN I compares as -inf).  The kernels above
// keep their code; these run only for symmetric_trees.
//
//   hist_scan_sym_kernel<NEWTON>   one workgroup per feature: each wave takes every fourth open node of a tile of
//                                  HIST_SYM_TILE and writes its terms per edge into LDS, then thread e adds the tile's terms
//                                  of edge e to its running I in node order; the last maximum over the edges as above
//   hist_sym_apply_kernel<NEWTON>  one wave per open node: the node's record under the level's winner (valid: it splits)

constexpr uint32_t HIST_SYM_TILE = 16;  // open nodes per LDS tile: 16 x 256 edges x (8 + 1) B = 36 KiB, four workgroups per CU

struct HistSymBestDev {
    double key;  // I of the feature's last-maximum candidate (-inf for a NaN I)
    uint32_t edge, valid;
};

// a node's unsplit term: (s s) / n, or the Newton term of its totals
template <bool NEWTON>
__device__ __forceinline__ double hist_sym_own(uint32_t n, long long qtot, long long wtot, int s_l, int s_w, double l2) {
    if (NEWTON) return hist_newton_term(qtot, ldexp((double)wtot, -s_w), s_l, l2);
    const double s = (double)qtot;
    return (s * s) / (double)n;
}

// t_a of one candidate: the importance hist_scan_kernel / hist_scan_newton_kernel give it where the node splits under it
// (*splits = true; under the Newton gain that includes gain > min_gain), else the node's own term
template <bool NEWTON>
__device__ __forceinline__ double hist_sym_term(uint32_t nl, uint32_t n, long long ql, long long wl, long long qtot, long long wtot,
                                                uint32_t min_leaf, int s_l, int s_w, double l2, double min_hess, double min_gain, double own,
                                                bool* splits) {
    *splits = false;
    const uint32_t nr = n - nl;
    if (nl == 0 || nr == 0 || nl < min_leaf || nr < min_leaf) return own;
    double imp;
    if (NEWTON) {
        const double hl = ldexp((double)wl, -s_w), hr = ldexp((double)(wtot - wl), -s_w);
        if (!(hl >= min_hess && hr >= min_hess && hl + l2 > 0.0 && hr + l2 > 0.0)) return own;
        imp = hist_newton_term(ql, hl, s_l, l2) + hist_newton_term(qtot - ql, hr, s_l, l2);
        if (!(imp - own > min_gain)) return own;
    } else {
        const double sl = (double)ql, sr = (double)(qtot - ql);
        imp = (sl * sl) / (double)nl + (sr * sr) / (double)nr;
    }
    *splits = true;
    return imp;
}

// grid F, 256 threads.  nodes[A]: the level's open nodes in order; best[f]
template <bool NEWTON>
__global__ __launch_bounds__(256) void hist_scan_sym_kernel(const HistItemDev* __restrict__ nodes, uint32_t A, uint32_t F, uint32_t k,
                                                            const uint32_t* __restrict__ nedges, const uint32_t* __restrict__ fsel,
                                                            const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ sum,
                                                            const unsigned long long* __restrict__ wsum, uint32_t min_leaf, int s_l, int s_w,
                                                            double l2, double min_hess, double min_gain, HistSymBestDev* __restrict__ best) {
    __shared__ double tile[HIST_SYM_TILE][HIST_MAX_BINS];
    __shared__ uint8_t took[HIST_SYM_TILE][HIST_MAX_BINS];
    __shared__ double red_key[4];
    __shared__ uint32_t red_j[4], red_have[4];
    const uint32_t f = blockIdx.x, e = threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t ne = min(nedges[fsel ? fsel[f] : f], k - 1);
    const uint32_t B = (k + 63) / 64;  // bins per lane (<= 4)
    double I = 0.0;
    uint32_t any = 0;
    for (uint32_t a0 = 0; a0 < A; a0 += HIST_SYM_TILE) {
        const uint32_t na = min(HIST_SYM_TILE, A - a0);
        for (uint32_t t = wave; t < na; t += 4) {  // (uniform in a wave: the shuffles below see all 64 lanes)
            const HistItemDev nd = nodes[a0 + t];
            const uint32_t n = nd.end - nd.begin;
            const size_t base = ((size_t)nd.slot * F + f) * k;
            uint32_t c[4];
            long long s[4], w[4];
            uint32_t tc = 0;
            long long ts = 0, tw = 0;
            for (uint32_t u = 0; u < 4; u++) {
                const uint32_t b = lane * B + u;
                const bool in = u < B && b < k;
                c[u] = in ? cnt[base + b] : 0u;
                s[u] = in ? (long long)sum[base + b] : 0ll;
                w[u] = NEWTON && in ? (long long)wsum[base + b] : 0ll;
                tc += c[u];
                ts += s[u];
                tw += w[u];
            }
            uint32_t ic = tc;
            long long is = ts, iw = tw;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t oc = __shfl_up(ic, o);
                const long long os = __shfl_up(is, o), ow = __shfl_up(iw, o);
                if ((int)lane >= o) {
                    ic += oc;
                    is += os;
                    iw += ow;
                }
            }
            const long long qtot = __shfl(is, 63), wtot = __shfl(iw, 63);
            const double own = hist_sym_own<NEWTON>(n, qtot, wtot, s_l, s_w, l2);
            uint32_t rc = ic - tc;  // counts / sums of the bins before this lane's
            long long rs = is - ts, rw = iw - tw;
            for (uint32_t u = 0; u < B; u++) {
                const uint32_t j = lane * B + u;
                rc += c[u];
                rs += s[u];
                rw += w[u];
                if (j >= ne) break;  // (ne <= 255: j stays inside the tile's row)
                bool sp;
                tile[t][j] = hist_sym_term<NEWTON>(rc, n, rs, rw, qtot, wtot, min_leaf, s_l, s_w, l2, min_hess, min_gain, own, &sp);
                took[t][j] = sp ? 1 : 0;
            }
        }
        __syncthreads();
        if (e < ne) {
            for (uint32_t t = 0; t < na; t++) {  // node order: the sum's order is the definition's
                const double term = tile[t][e];
                I = (a0 + t == 0) ? term : I + term;
                any |= took[t][e];
            }
        }
        __syncthreads();
    }
    // the last maximum over the edges: larger key, then the later edge
    double wkey = (I != I) ? -INFINITY : I;
    uint32_t wj = e, whave = (e < ne && any) ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) {
        const double okey = __shfl_xor(wkey, o);
        const uint32_t oj = __shfl_xor(wj, o), ohave = __shfl_xor(whave, o);
        if (ohave && (!whave || okey > wkey || (okey == wkey && oj > wj))) {
            whave = 1;
            wkey = okey;
            wj = oj;
        }
    }
    if (lane == 0) {
        red_key[wave] = wkey;
        red_j[wave] = wj;
        red_have[wave] = whave;
    }
    __syncthreads();
    if (e == 0) {
        for (uint32_t v = 1; v < 4; v++) {
            if (red_have[v] && (!whave || red_key[v] > wkey || (red_key[v] == wkey && red_j[v] > wj))) {
                whave = 1;
                wkey = red_key[v];
                wj = red_j[v];
            }
        }
        best[f] = whave ? HistSymBestDev{wkey, wj, 1u} : HistSymBestDev{0.0, 0u, 0u};
    }
}

// grid A, one wave per open node; f: the winner's index among the tree's F, j: its edge.  out[a]: node a's record under the
// winner (wl, wtot: 0 under the variance criterion)
template <bool NEWTON>
__global__ __launch_bounds__(64) void hist_sym_apply_kernel(const HistItemDev* __restrict__ nodes, uint32_t F, uint32_t k, uint32_t f, uint32_t j,
                                                            const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ sum,
                                                            const unsigned long long* __restrict__ wsum, uint32_t min_leaf, int s_l, int s_w,
                                                            double l2, double min_hess, double min_gain, HistBestNewtonDev* __restrict__ out) {
    const uint32_t a = blockIdx.x, lane = threadIdx.x;
    const HistItemDev nd = nodes[a];
    const uint32_t n = nd.end - nd.begin;
    const size_t base = ((size_t)nd.slot * F + f) * k;
    uint32_t nl = 0;
    long long ql = 0, wl = 0, qtot = 0, wtot = 0;
    for (uint32_t b = lane; b < k; b += 64) {
        const uint32_t c = cnt[base + b];
        const long long s = (long long)sum[base + b], w = NEWTON ? (long long)wsum[base + b] : 0ll;
        qtot += s;
        wtot += w;
        if (b <= j) {
            nl += c;
            ql += s;
            wl += w;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {  // (integer sums: any order)
        nl += __shfl_xor(nl, o);
        ql += __shfl_xor(ql, o);
        wl += __shfl_xor(wl, o);
        qtot += __shfl_xor(qtot, o);
        wtot += __shfl_xor(wtot, o);
    }
    if (lane != 0) return;
    const double own = hist_sym_own<NEWTON>(n, qtot, wtot, s_l, s_w, l2);
    bool sp;
    const double imp = hist_sym_term<NEWTON>(nl, n, ql, wl, qtot, wtot, min_leaf, s_l, s_w, l2, min_hess, min_gain, own, &sp);
    out[a] = HistBestNewtonDev{imp, ql, qtot, wl, wtot, j, nl, sp ? 1u : 0u, 0u};
}
