// Part of device.hip (single translation unit; see that file's header).  Permutation importance (DESIGN.md section 16; permute.hpp
// states the definition): the scores of a model on the dataset with ONE column read from other rows, for a chunk of columns
// and every repeat at once.  Score slot (k * R + r) of `out` = the scores on D_{feats[k], r}.
//
// Both kernels: block = one 64-document tile (the trees kernel: four waves on it), lane = document, the tile's rows staged in LDS at row stride 4 dq + 1 dwords (as
// tree_ensemble_kernel<true, .> stages them; ROWS_IN_LDS = false reads the tiles where 64 (4 dq + 1) 4 bytes do not fit).  The
// substitute value of (document, column f, repeat r) is gathered from the column-major copy where the dataset has one, else
// from the tiles.  Every position a launch visits gets a score (padding and the documents of a view's parent included:
// src maps them to themselves); nothing reads those.

struct PermArgs {
    const float* xb;
    PosMap pm;
    uint32_t dq, d, np;
    const float* xcol;      // [d][np], or nullptr: gather from the tiles
    const uint32_t* src;    // [R][np] the position whose value position p reads in repeat r
    const uint32_t* feats;  // [nf] ascending, every one < d
    uint32_t nf, R, r0;     // this launch takes repeats r0 .. r0 + (its count) - 1
    double* out;
};

__device__ __forceinline__ float perm_gather(const PermArgs& a, uint32_t r, uint32_t p, uint32_t f) {
    const uint32_t sp = a.src[(size_t)r * a.np + p];
    return a.xcol != nullptr ? a.xcol[(size_t)f * a.np + sp] : a.xb[xb_index(sp, f, a.dq)];
}

// (quads first, first + step, ..: the waves of a block that share one tile's rows stage a part each)
__device__ __forceinline__ void perm_stage_rows(const float* __restrict__ xb, uint32_t p, uint32_t dq, float* __restrict__ myrow, uint32_t first = 0,
                                                uint32_t step = 1) {
    const float4* xp = (const float4*)xb + (size_t)(p >> 6) * dq * 64 + (p & 63);
    for (uint32_t j4 = first; j4 < dq; j4 += step) {
        const float4 v = xp[(size_t)j4 * 64];
        float* r = myrow + j4 * 4;
        r[0] = v.x;
        r[1] = v.y;
        r[2] = v.z;
        r[3] = v.w;
    }
}

// Linear: s = sum_j f64(x'[j]) * w[j], j ascending, unfused, with x'[f] the substitute.  One sweep over the listed columns keeps
// the running prefix (the same ordered sum up to f - 1); per column, RC repeats continue from prefix + f64(v_r) * w[f] through
// the tail f + 1 .. 4 dq - 1, whose products do not depend on r.  w arrives zero-padded to 4 dq, as score_linear_kernel's.
template <bool ROWS_IN_LDS, int RC>
__global__ __launch_bounds__(64) void permute_linear_kernel(PermArgs a, const double* __restrict__ w) {
    extern __shared__ float perm_rows[];  // [64][4*dq+1]
    const uint32_t tid = threadIdx.x;
    const uint32_t pv = posmap_at(a.pm, blockIdx.x * 64u + tid);  // (whole tiles: always a position)
    const uint32_t p = pv != IDX_INVALID ? pv : 0u;
    const uint32_t dp = a.dq * 4;
    float* myrow = perm_rows + tid * (dp + 1);
    if (ROWS_IN_LDS) {
        perm_stage_rows(a.xb, p, a.dq, myrow);
        __syncthreads();
    }
    auto x = [&](uint32_t j) -> double { return (double)(ROWS_IN_LDS ? myrow[j] : a.xb[xb_index(p, j, a.dq)]); };
    double prefix = 0.0;
    uint32_t j = 0;
    for (uint32_t k = 0; k < a.nf; k++) {
        const uint32_t f = a.feats[k];
        for (; j < f; j++) {
            const double prod = x(j) * w[j];
            prefix = prefix + prod;
        }
        double s[RC];
        const double wf = w[f];
#pragma unroll
        for (int r = 0; r < RC; r++) {
            const double prod = (double)perm_gather(a, a.r0 + r, p, f) * wf;
            s[r] = prefix + prod;
        }
#pragma unroll 8
        for (uint32_t jj = f + 1; jj < dp; jj++) {
            const double prod = x(jj) * w[jj];
#pragma unroll
            for (int r = 0; r < RC; r++) s[r] = s[r] + prod;
        }
        if (pv != IDX_INVALID) {
#pragma unroll
            for (int r = 0; r < RC; r++) a.out[((size_t)k * a.R + a.r0 + r) * a.np + p] = s[r];
        }
    }
}

// Trees (nodes as tree_ensemble_kernel's: children adjacent): per listed column, up to ACC = 8 repeats in registers.  Trees in
// order; bit k of uses[t * uw ..] says whether tree t splits on feats[k] (the same for the whole block): if not, one walk of the
// document's own row and acc[r] = acc[r] + w_t leaf for every r; otherwise one walk per repeat, the row's value of that column
// replaced by v_r through a select.  raw_single (one bare DecisionTree): the leaf itself.  fid >= d reads 0.0.
// The walks wait on node loads, and the staged rows cap a CU at four tiles: PERM_TREE_WAVES waves share a tile's rows and take
// every PERM_TREE_WAVES-th listed column each (a wave's control flow stays uniform; what a (document, column, repeat) adds up
// does not depend on which wave does it).
constexpr int PERM_TREE_WAVES = 4;
template <bool ROWS_IN_LDS>
__global__ __launch_bounds__(64 * PERM_TREE_WAVES) void permute_trees_kernel(PermArgs a, const TreeNodeDev* __restrict__ nodes, const int32_t* __restrict__ roots,
                                                           const double* __restrict__ tw, uint32_t ntrees, int raw_single,
                                                           const uint32_t* __restrict__ uses, uint32_t uw, uint32_t rc) {
    constexpr int ACC = (int)frpermute::ACC;
    extern __shared__ float perm_rows[];  // [64][4*dq+1]
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t pv = posmap_at(a.pm, blockIdx.x * 64u + lane);  // (whole tiles: always a position)
    const uint32_t p = pv != IDX_INVALID ? pv : 0u;
    float* myrow = perm_rows + lane * (a.dq * 4 + 1);
    if (ROWS_IN_LDS) {
        perm_stage_rows(a.xb, p, a.dq, myrow, wave, PERM_TREE_WAVES);
        __syncthreads();
    }
    auto x = [&](uint32_t fid) -> float { return ROWS_IN_LDS ? myrow[fid] : a.xb[xb_index(p, fid, a.dq)]; };
    for (uint32_t k = wave; k < a.nf; k += PERM_TREE_WAVES) {
        const uint32_t f = a.feats[k];
        float v[ACC];
        double acc[ACC];
#pragma unroll
        for (int r = 0; r < ACC; r++) {
            v[r] = (uint32_t)r < rc ? perm_gather(a, a.r0 + r, p, f) : 0.0f;
            acc[r] = 0.0;
        }
        for (uint32_t t = 0; t < ntrees; t++) {
            const bool used = (uses[(size_t)t * uw + (k >> 5)] >> (k & 31)) & 1u;
            if (!used) {
                TreeNodeDev nd = nodes[roots[t]];
                while (__any(nd.fid >= 0)) {
                    if (nd.fid >= 0) {
                        const float xv = (uint32_t)nd.fid < a.d ? x((uint32_t)nd.fid) : 0.0f;  // Features::get -> None -> unwrap_or(0.0)
                        nd = nodes[((double)xv <= nd.split) ? nd.lhs : nd.lhs + 1];
                    }
                }
                const double prod = tw[t] * nd.split;
#pragma unroll
                for (int r = 0; r < ACC; r++) acc[r] = raw_single ? nd.split : acc[r] + prod;
            } else {
                TreeNodeDev nd[ACC];
                const TreeNodeDev root = nodes[roots[t]];
#pragma unroll
                for (int r = 0; r < ACC; r++) {
                    nd[r] = root;
                    if ((uint32_t)r >= rc) nd[r].fid = -1;  // (no repeat here: nothing to walk, nothing stored)
                }
                bool any_inner = true;
                while (any_inner) {
                    any_inner = false;
#pragma unroll
                    for (int r = 0; r < ACC; r++) {
                        if (nd[r].fid >= 0) {
                            const uint32_t fid = (uint32_t)nd[r].fid;
                            float xv = 0.0f;
                            if (fid < a.d) {
                                const float own = x(fid);
                                xv = fid == f ? v[r] : own;
                            }
                            nd[r] = nodes[((double)xv <= nd[r].split) ? nd[r].lhs : nd[r].lhs + 1];
                            any_inner |= nd[r].fid >= 0;
                        }
                    }
                    any_inner = __any(any_inner);
                }
                const double wt = tw[t];
#pragma unroll
                for (int r = 0; r < ACC; r++) {
                    const double prod = wt * nd[r].split;
                    acc[r] = raw_single ? nd[r].split : acc[r] + prod;
                }
            }
        }
        if (pv != IDX_INVALID) {
#pragma unroll
            for (int r = 0; r < ACC; r++)
                if ((uint32_t)r < rc) a.out[((size_t)k * a.R + a.r0 + r) * a.np + p] = acc[r];
        }
    }
}

// SingleFeature (src/model.rs:35-40): dir * f64(x'[fid]); a listed column other than fid leaves the scores as they are, and
// fid >= d reads 0.0.  grid (positions / 256, nf * R).
__global__ __launch_bounds__(256) void permute_single_kernel(PermArgs a, uint32_t fid, double dir) {
    const uint32_t p = posmap_position(a.pm);
    if (p == IDX_INVALID) return;
    const uint32_t slot = blockIdx.y, k = slot / a.R, r = slot % a.R;
    float xv = 0.0f;
    if (fid < a.d) xv = a.feats[k] == fid ? perm_gather(a, r, p, fid) : a.xb[xb_index(p, fid, a.dq)];
    a.out[(size_t)slot * a.np + p] = dir * (double)xv;
}

// acc = acc + w * t (unfused) per slot: axpy_unfused_kernel over B slots.  grid (positions / 256, B).
__global__ __launch_bounds__(256) void permute_axpy_kernel(double* __restrict__ acc, const double* __restrict__ t, PosMap pm, uint32_t np, double w) {
    const uint32_t p = posmap_position(pm);
    if (p == IDX_INVALID) return;
    const size_t i = (size_t)blockIdx.y * np + p;
    const double prod = w * t[i];
    acc[i] = acc[i] + prod;
}
