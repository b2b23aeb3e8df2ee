// Model explanation: exact per-document feature contributions of tree models (path-dependent
// TreeSHAP).  A translation unit of its own, like fullverify.hip: device.o is built from its own sources and none of its
// kernels moves.  Three kernels:
//   explain_cover_kernel    routes the background's documents through every tree and counts them per leaf (integer atomics)
//   explain_kernel          a lane owns a document, a one-wave workgroup walks the path table in uniform control flow
//   explain_abs_tile_kernel / explain_abs_sum_kernel   the sum of |phi| per column, in a fixed shape
#include "explain.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

namespace frdev {

#define EX_HIP(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            if (err) *err = std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr; \
            return false;                                                                   \
        }                                                                                   \
    } while (0)

namespace {

// the tile layout of kernels_score.inc (xb_index)
__device__ __forceinline__ size_t ex_xb_index(uint32_t p, uint32_t j, uint32_t dq) {
    return ((size_t)(p >> 6) * dq + (j >> 2)) * 256 + (size_t)(p & 63) * 4 + (j & 3);
}

template <typename T>
struct ExBuf {
    T* p = nullptr;
    ~ExBuf() {
        if (p) (void)hipFree(p);
    }
    bool alloc(size_t n, std::string* err) {
        EX_HIP(hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)));
        return true;
    }
    bool upload(const std::vector<T>& v, std::string* err) {
        if (!alloc(v.size(), err)) return false;
        if (!v.empty()) EX_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return true;
    }
};

struct ExTimer {
    hipEvent_t a = nullptr, b = nullptr;
    ~ExTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    bool begin(std::string* err) {
        if (!a) EX_HIP(hipEventCreate(&a));
        if (!b) EX_HIP(hipEventCreate(&b));
        EX_HIP(hipEventRecord(a, nullptr));
        return true;
    }
    bool end(double* ms_total, std::string* err) {
        EX_HIP(hipEventRecord(b, nullptr));
        EX_HIP(hipEventSynchronize(b));
        float ms = 0.0f;
        EX_HIP(hipEventElapsedTime(&ms, a, b));
        *ms_total += (double)ms;
        return true;
    }
};

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// Covers.  Workgroup (bx, t) takes every gridDim.x-th stretch of 256 documents through tree t.  A tree of at most
// EX_COVER_LDS leaves is counted in LDS first and handed over with one atomic per (workgroup, leaf that was reached);
// a larger one adds to the global counters directly.  Sums of integers: whatever the order, the same counts.
// ------------------------------------------------------------------------------------------------------------------
constexpr uint32_t EX_COVER_LDS = 4096;
constexpr uint32_t EX_COVER_GRID = 256;

__global__ __launch_bounds__(256) void explain_cover_kernel(const float* __restrict__ xb, uint32_t dq, uint32_t d, const uint32_t* __restrict__ pos,
                                                            uint32_t n, const int32_t* __restrict__ nfid, const int32_t* __restrict__ nlhs,
                                                            const int32_t* __restrict__ nrhs, const double* __restrict__ nsplit,
                                                            const int32_t* __restrict__ roots, const uint32_t* __restrict__ leaf0,
                                                            uint32_t* __restrict__ counts) {
    __shared__ uint32_t local[EX_COVER_LDS];
    const uint32_t t = blockIdx.y;
    const uint32_t l0 = leaf0[t], nl = leaf0[t + 1] - l0;
    const bool in_lds = nl <= EX_COVER_LDS;
    if (in_lds) {
        for (uint32_t j = threadIdx.x; j < nl; j += 256) local[j] = 0u;
        __syncthreads();
    }
    const int32_t root = roots[t];
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t p = pos[i];
        int32_t k = root;
        int32_t f = nfid[k];
        while (f >= 0) {
            const float xv = (uint32_t)f < d ? xb[ex_xb_index(p, (uint32_t)f, dq)] : 0.0f;
            k = ((double)xv <= nsplit[k]) ? nlhs[k] : nrhs[k];
            f = nfid[k];
        }
        const uint32_t leaf = (uint32_t)nlhs[k] - l0;  // (< nl: the host numbered them)
        if (leaf < nl) {
            if (in_lds) atomicAdd(&local[leaf], 1u);
            else atomicAdd(&counts[l0 + leaf], 1u);
        }
    }
    if (in_lds) {
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < nl; j += 256)
            if (local[j]) atomicAdd(&counts[l0 + j], local[j]);
    }
}

bool explain_covers(const ExDocs& B, const ExWalk& walk, std::vector<uint32_t>* counts, ExTimes* times, std::string* err) {
    const size_t T = walk.root.size(), L = walk.leaf0.empty() ? 0 : walk.leaf0.back();
    counts->assign(L, 0u);
    if (T == 0 || B.pos.empty()) return true;
    EX_HIP(hipSetDevice(B.device));
    ExBuf<uint32_t> pos, leaf0, cnt;
    ExBuf<int32_t> fid, lhs, rhs, roots;
    ExBuf<double> split;
    if (!pos.upload(B.pos, err) || !leaf0.upload(walk.leaf0, err) || !fid.upload(walk.fid, err) || !lhs.upload(walk.lhs, err) ||
        !rhs.upload(walk.rhs, err) || !roots.upload(walk.root, err) || !split.upload(walk.split, err) || !cnt.alloc(L, err))
        return false;
    EX_HIP(hipMemset(cnt.p, 0, std::max<size_t>(L, 1) * sizeof(uint32_t)));
    ExTimer tm;
    if (!tm.begin(err)) return false;
    const uint32_t n = (uint32_t)B.pos.size();
    const uint32_t gx = std::min<uint32_t>((n + 255u) / 256u, EX_COVER_GRID);
    for (size_t t0 = 0; t0 < T; t0 += 65535) {  // (gridDim.y)
        const uint32_t nt = (uint32_t)std::min<size_t>(T - t0, 65535);
        explain_cover_kernel<<<dim3(gx, nt), 256>>>(B.xb, B.dq, B.d, pos.p, n, fid.p, lhs.p, rhs.p, split.p, roots.p + t0, leaf0.p + t0, cnt.p);
        EX_HIP(hipGetLastError());
    }
    ExTimes scratch;
    if (!tm.end(times ? &times->kernel_ms : &scratch.kernel_ms, err)) return false;
    EX_HIP(hipMemcpy(counts->data(), cnt.p, L * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return true;
}

// ------------------------------------------------------------------------------------------------------------------
// Contributions.  One wave per workgroup: lane = document, tile = blockIdx.x (+ tile0), everything else uniform.
//
// Per tree: the lane's values of the tree's features go to LDS (xs[slot][lane]) and the tree's accumulators c[slot][lane]
// are zeroed.  Per leaf, depth first: bit e of `obits` = lo_e < (double)x <= hi_e.  For every element i of the leaf's m:
//   W[0] = 1; l = 0
//   for every other element e, ascending:  l = l + 1; carry = 0
//       for j = l - 1 .. 0:  w = W[j]; W[j + 1] = carry + (o_e * w) * fo[l][j]; carry = (z_e * w) * fz[l][j]
//       W[0] = carry
//   sum = 0; for j = 0 .. m - 1: sum = sum + W[j]
//   c[slot_i] = c[slot_i] + ((sum * (o_i - z_i)) * leaf)
// (EXTEND over the other m - 1 elements instead of an UNWIND of element i: no division, so a zero or tiny cover ratio costs
// nothing -- DESIGN.md section 12.)  After the tree: phi[col] = phi[col] + w_t * c[slot], product and sum rounded separately.
// For a leaf of more than EX_REG_PATH elements W is [m + 1][64] in LDS, lane-major: whatever j, lane L reads bank pair L;
// shorter paths keep W in registers (ex_leaf_regs).  Output: out[(tile * ncols + col) * 64 + lane].
// ------------------------------------------------------------------------------------------------------------------
struct ExArgs {
    const float* xb;
    const uint32_t* pos;
    const uint32_t *leaf0, *feat0, *m, *eoff, *slot, *fid, *col;
    const double *weight, *value, *lo, *hi, *z, *fo, *fz;
    double* out;
    uint32_t dq, d, n, trees, ncols, max_path, max_tree_feats, tile0;
};

// One leaf of M <= EX_REG_PATH elements with the permutation weights in registers: the loops of the comment above, fully
// unrolled (l, j and the two quotients are compile-time constants), the same operations in the same order -- the same bits
// as the LDS form below, which takes the longer paths.
template <int M>
__device__ __forceinline__ void ex_leaf_regs(const ExArgs& a, uint32_t e0, uint32_t obits, double leaf, double* C) {
    double z[M], o[M];
#pragma unroll
    for (int e = 0; e < M; e++) {
        z[e] = a.z[e0 + e];
        o[e] = ((obits >> e) & 1u) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < M; k++) {
        double W[M];
        W[0] = 1.0;
#pragma unroll
        for (int e = 0; e < M; e++) {
            if (e == k) continue;
            const int l = e < k ? e + 1 : e;
            double carry = 0.0;
#pragma unroll
            for (int j = l - 1; j >= 0; j--) {
                const double w = W[j];
                const double ow = o[e] * w;
                const double up = ow * ((double)(j + 1) / (double)(l + 1));
                W[j + 1] = carry + up;
                const double zw = z[e] * w;
                carry = zw * ((double)(l - j) / (double)(l + 1));
            }
            W[0] = carry;
        }
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < M; j++) sum = sum + W[j];
        const double diff = o[k] - z[k];
        const double sd = sum * diff;
        const double add = sd * leaf;
        double* c = C + a.slot[e0 + k] * 64;
        *c = *c + add;
    }
}

__global__ __launch_bounds__(64) void explain_kernel(ExArgs a) {
    extern __shared__ double ex_lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t wrows = ex_w_rows(a.max_path);
    double* W = ex_lds + lane;                                            // W[j * 64]
    double* C = ex_lds + (size_t)wrows * 64 + lane;                       // C[slot * 64]
    float* XS = (float*)(ex_lds + (size_t)(wrows + a.max_tree_feats) * 64) + lane;  // XS[slot * 64]
    const uint32_t i = (a.tile0 + blockIdx.x) * 64 + lane;
    const uint32_t p = a.pos[i < a.n ? i : a.n - 1];  // (a lane past the end explains the last document again; nobody reads it)
    double* out = a.out + (size_t)blockIdx.x * a.ncols * 64 + lane;
    for (uint32_t c = 0; c < a.ncols; c++) out[(size_t)c * 64] = 0.0;
    for (uint32_t t = 0; t < a.trees; t++) {
        const uint32_t f0 = a.feat0[t], nf = a.feat0[t + 1] - f0;
        for (uint32_t s = 0; s < nf; s++) {
            const uint32_t fid = a.fid[f0 + s];
            XS[s * 64] = fid < a.d ? a.xb[ex_xb_index(p, fid, a.dq)] : 0.0f;
            C[s * 64] = 0.0;
        }
        const uint32_t l1 = a.leaf0[t + 1];
        for (uint32_t L = a.leaf0[t]; L < l1; L++) {
            const uint32_t m = a.m[L], e0 = a.eoff[L];
            const double leaf = a.value[L];
            uint32_t obits = 0;
            for (uint32_t e = 0; e < m; e++) {
                const double x = (double)XS[a.slot[e0 + e] * 64];
                const bool o = (a.lo[e0 + e] < x) && (x <= a.hi[e0 + e]);
                obits |= (o ? 1u : 0u) << e;
            }
            switch (m) {  // (uniform)
                case 1: ex_leaf_regs<1>(a, e0, obits, leaf, C); continue;
                case 2: ex_leaf_regs<2>(a, e0, obits, leaf, C); continue;
                case 3: ex_leaf_regs<3>(a, e0, obits, leaf, C); continue;
                case 4: ex_leaf_regs<4>(a, e0, obits, leaf, C); continue;
                case 5: ex_leaf_regs<5>(a, e0, obits, leaf, C); continue;
                case 6: ex_leaf_regs<6>(a, e0, obits, leaf, C); continue;
                case 7: ex_leaf_regs<7>(a, e0, obits, leaf, C); continue;
                case 8: ex_leaf_regs<8>(a, e0, obits, leaf, C); continue;
                default: break;
            }
            for (uint32_t k = 0; k < m; k++) {
                W[0] = 1.0;
                uint32_t l = 0;
                for (uint32_t e = 0; e < m; e++) {
                    if (e == k) continue;
                    l++;
                    const double oe = ((obits >> e) & 1u) ? 1.0 : 0.0;
                    const double ze = a.z[e0 + e];
                    const double* fo = a.fo + l * 33;
                    const double* fz = a.fz + l * 33;
                    double carry = 0.0;
                    for (uint32_t j = l; j-- > 0;) {
                        const double w = W[j * 64];
                        const double ow = oe * w;
                        const double up = ow * fo[j];
                        W[(j + 1) * 64] = carry + up;
                        const double zw = ze * w;
                        carry = zw * fz[j];
                    }
                    W[0] = carry;
                }
                double sum = 0.0;
                for (uint32_t j = 0; j < m; j++) sum = sum + W[j * 64];
                const double ok = ((obits >> k) & 1u) ? 1.0 : 0.0;
                const double diff = ok - a.z[e0 + k];
                const double sd = sum * diff;
                const double add = sd * leaf;
                double* c = C + a.slot[e0 + k] * 64;
                *c = *c + add;
            }
        }
        const double wt = a.weight[t];
        for (uint32_t s = 0; s < nf; s++) {
            const double prod = wt * C[s * 64];
            double* o = out + (size_t)a.col[f0 + s] * 64;
            *o = *o + prod;
        }
    }
}

// part[(tile * ncols + c)] = the sum of |phi_c| over the tile's lanes that hold a document, in lane order
__global__ __launch_bounds__(256) void explain_abs_tile_kernel(const double* __restrict__ out, uint32_t ncols, uint32_t tiles, uint32_t tile0,
                                                               uint32_t n, double* __restrict__ part) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= tiles * ncols) return;
    const uint32_t tile = k / ncols;
    const uint32_t first = (tile0 + tile) * 64;
    const uint32_t lanes = n - first < 64u ? n - first : 64u;
    const double* v = out + (size_t)k * 64;
    double s = 0.0;
    for (uint32_t j = 0; j < lanes; j++) s = s + fabs(v[j]);
    part[k] = s;
}

// total[c] = total[c] + part[tile][c], tiles ascending: one running sum per column over all the tiles of all the launches
__global__ __launch_bounds__(64) void explain_abs_sum_kernel(const double* __restrict__ part, uint32_t ncols, uint32_t tiles, double* __restrict__ total) {
    const uint32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c >= ncols) return;
    double s = total[c];
    for (uint32_t t = 0; t < tiles; t++) s = s + part[(size_t)t * ncols + c];
    total[c] = s;
}

void explain_factors(std::vector<double>* fo, std::vector<double>* fz) {
    fo->assign(33 * 33, 0.0), fz->assign(33 * 33, 0.0);
    for (uint32_t l = 1; l <= EX_MAX_PATH; l++)
        for (uint32_t j = 0; j < l; j++) {
            (*fo)[l * 33 + j] = (double)(j + 1) / (double)(l + 1);
            (*fz)[l * 33 + j] = (double)(l - j) / (double)(l + 1);
        }
}

namespace {

struct ExDevice {
    ExBuf<uint32_t> pos, leaf0, feat0, m, eoff, slot, fid, col;
    ExBuf<double> weight, value, lo, hi, z, fo, fz;
    ExArgs a{};
    size_t lds = 0;
    bool upload(const ExDocs& X, const ExTables& tab, std::string* err) {
        if (tab.max_path > EX_MAX_PATH) {
            if (err) *err = "a path of " + std::to_string(tab.max_path) + " distinct features is longer than the explain kernel supports (32)";
            return false;
        }
        lds = ex_lds_bytes(tab.max_path, tab.max_tree_feats);
        if (lds > EX_LDS_MAX) {
            if (err)
                *err = "a tree that splits on " + std::to_string(tab.max_tree_feats) + " distinct features needs " + std::to_string(lds) +
                       " bytes of LDS per wave, the explain kernel has " + std::to_string(EX_LDS_MAX);
            return false;
        }
        std::vector<double> fo_h, fz_h;
        explain_factors(&fo_h, &fz_h);
        if (!pos.upload(X.pos, err) || !leaf0.upload(tab.leaf0, err) || !feat0.upload(tab.feat0, err) || !m.upload(tab.m, err) ||
            !eoff.upload(tab.eoff, err) || !slot.upload(tab.slot, err) || !fid.upload(tab.fid, err) || !col.upload(tab.col, err) ||
            !weight.upload(tab.weight, err) || !value.upload(tab.value, err) || !lo.upload(tab.lo, err) || !hi.upload(tab.hi, err) ||
            !z.upload(tab.z, err) || !fo.upload(fo_h, err) || !fz.upload(fz_h, err))
            return false;
        a.xb = X.xb, a.pos = pos.p;
        a.leaf0 = leaf0.p, a.feat0 = feat0.p, a.m = m.p, a.eoff = eoff.p, a.slot = slot.p, a.fid = fid.p, a.col = col.p;
        a.weight = weight.p, a.value = value.p, a.lo = lo.p, a.hi = hi.p, a.z = z.p, a.fo = fo.p, a.fz = fz.p;
        a.dq = X.dq, a.d = X.d, a.n = (uint32_t)X.pos.size(), a.trees = (uint32_t)tab.weight.size(), a.ncols = tab.ncols;
        a.max_path = tab.max_path, a.max_tree_feats = tab.max_tree_feats;
        // (more than the default 64 KB of dynamic LDS has to be asked for, per device: fullverify.hip)
        if (lds > ((size_t)48 << 10)) EX_HIP(hipFuncSetAttribute((const void*)explain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        return true;
    }
    bool launch(uint32_t tile0, uint32_t tiles, double* out, std::string* err) {
        a.tile0 = tile0, a.out = out;
        explain_kernel<<<tiles, 64, lds>>>(a);
        EX_HIP(hipGetLastError());
        return true;
    }
};

}  // namespace

bool explain_values(const ExDocs& X, const ExTables& tab, size_t budget, std::vector<double>* phi, ExTimes* times, std::string* err) {
    const size_t n = X.pos.size(), nc = tab.ncols;
    phi->assign(n * nc, 0.0);
    if (n == 0 || nc == 0) return true;
    EX_HIP(hipSetDevice(X.device));
    const size_t tiles = (n + 63) / 64, need = tiles * nc * 64 * sizeof(double);
    if (need > budget || tiles > 0x3FFFFFFu) {
        if (err)
            *err = "the contributions of " + std::to_string(n) + " documents x " + std::to_string(nc) + " features need " + std::to_string(need) +
                   " bytes on the device, " + std::to_string(budget) + " are free: explain a sampled view, or ask for feature_importance";
        return false;
    }
    ExDevice dev;
    if (!dev.upload(X, tab, err)) return false;
    ExBuf<double> out;
    if (!out.alloc(tiles * nc * 64, err)) return false;
    ExTimes scratch;
    ExTimes* tt = times ? times : &scratch;
    ExTimer tm;
    if (!tm.begin(err) || !dev.launch(0, (uint32_t)tiles, out.p, err) || !tm.end(&tt->kernel_ms, err)) return false;
    std::vector<double> tmp(tiles * nc * 64);
    if (!tm.begin(err)) return false;
    EX_HIP(hipMemcpy(tmp.data(), out.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (!tm.end(&tt->copy_ms, err)) return false;
    for (size_t i = 0; i < n; i++)
        for (size_t c = 0; c < nc; c++) (*phi)[i * nc + c] = tmp[((i >> 6) * nc + c) * 64 + (i & 63)];
    return true;
}

bool explain_sum_abs(const ExDocs& X, const ExTables& tab, std::vector<double>* sum_abs, ExTimes* times, std::string* err) {
    const size_t n = X.pos.size(), nc = tab.ncols;
    sum_abs->assign(nc, 0.0);
    if (n == 0 || nc == 0) return true;
    EX_HIP(hipSetDevice(X.device));
    const size_t tiles = (n + 63) / 64;
    if (tiles > 0x3FFFFFFu) {
        if (err) *err = "too many documents for the explain kernel's 32-bit document index";
        return false;
    }
    const size_t chunk = std::min<size_t>(tiles, EX_CHUNK_TILES);
    ExDevice dev;
    if (!dev.upload(X, tab, err)) return false;
    ExBuf<double> out, part, total;
    if (!out.alloc(chunk * nc * 64, err) || !part.alloc(chunk * nc, err) || !total.alloc(nc, err)) return false;
    EX_HIP(hipMemset(total.p, 0, nc * sizeof(double)));
    ExTimes scratch;
    ExTimes* tt = times ? times : &scratch;
    ExTimer tm;
    if (!tm.begin(err)) return false;
    for (size_t t0 = 0; t0 < tiles; t0 += chunk) {
        const uint32_t nt = (uint32_t)std::min(chunk, tiles - t0);
        if (!dev.launch((uint32_t)t0, nt, out.p, err)) return false;
        explain_abs_tile_kernel<<<(nt * (uint32_t)nc + 255u) / 256u, 256>>>(out.p, (uint32_t)nc, nt, (uint32_t)t0, (uint32_t)n, part.p);
        EX_HIP(hipGetLastError());
        explain_abs_sum_kernel<<<((uint32_t)nc + 63u) / 64u, 64>>>(part.p, (uint32_t)nc, nt, total.p);
        EX_HIP(hipGetLastError());
    }
    if (!tm.end(&tt->kernel_ms, err)) return false;
    EX_HIP(hipMemcpy(sum_abs->data(), total.p, nc * sizeof(double), hipMemcpyDeviceToHost));
    return true;
}

}  // namespace frdev
