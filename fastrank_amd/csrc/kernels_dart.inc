// Part of device.hip (single translation unit; see that file's header).  LambdaMART's DART boosting (DESIGN.md section 11,
// "DART"): the leaf cache and the kernel that re-forms the scores from it.
//
// leaf[t * stride + i] (u16) = the leaf, in depth-first numbering, that the document at LOGICAL index i (PosMap: a sampled
// view counts its own tiles only) reaches in tree t; vals[voff[t] + leaf] (f64) = that leaf's value.  stride = the number of
// logical indices, a multiple of 64.

constexpr int DART_DOCS = 4;                                // adjacent documents per lane: one 8-byte load of four u16 per tree
constexpr int DART_BLOCK = 256;                             // threads per workgroup: a tile of 1024 documents
constexpr uint32_t DART_MAX_GRID = 1024;                    // workgroups of a re-forming: each takes every DART_MAX_GRID-th tile
constexpr uint32_t DART_LDS_VALUES = 64 * 1024 / 8;         // the leaf values are gathered from LDS while all of them fit 64 KiB
constexpr uint32_t DART_MAX_LEAVES = 65536;

// row[i] = the leaf number score slot 0 holds for logical index i (the tree-scoring kernel run on a copy of the tree whose
// leaves hold their own index).  A value that is no leaf number of the tree is stored as leaf 0 and raises *bad: every entry
// of the cache stays inside its tree's stretch of the value table.
__global__ __launch_bounds__(256) void dart_fill_kernel(const double* __restrict__ scores, PosMap pm, uint32_t stride, uint32_t n_leaves,
                                                        const uint32_t* __restrict__ perm, uint16_t* __restrict__ row, int* __restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= stride) return;
    const uint32_t p = posmap_at(pm, i);
    if (p == IDX_INVALID) return;
    const double v = scores[p];
    const bool ok = v >= 0.0 && v < (double)n_leaves;
    row[i] = ok ? (uint16_t)(uint32_t)v : (uint16_t)0;
    if (!ok && perm[p] != IDX_INVALID) atomicOr(bad, 1);  // (a padding position holds no document: whatever it scored, leaf 0)
}

// s = +0.0; for k ascending: t = trees[k]; s = s + w[t] * vals[voff[t] + leaf[t][i]], product and sum rounded separately (the
// WeightedEnsemble recurrence over the listed trees: the order across trees is fixed, so the parallelism is across documents).
// A lane takes DART_DOCS adjacent logical indices -- they share a 64-position tile, so their positions are adjacent too --
// and walks the trees in the inner loop: per tree one 8-byte load per lane, 512 contiguous bytes per wave, and four gathers
// of leaf values, from LDS (LDS_VALS: the workgroup copies the whole table there once and then takes tile after tile of
// 1024 documents) or from global memory.  Writes score slot 0 and the ensemble accumulator.
template <bool LDS_VALS>
__global__ __launch_bounds__(DART_BLOCK) void dart_rescore_kernel(const uint16_t* __restrict__ leaf, uint32_t stride,
                                                                  const double* __restrict__ vals, const uint32_t* __restrict__ voff,
                                                                  uint32_t n_vals, const double* __restrict__ w,
                                                                  const uint32_t* __restrict__ trees, uint32_t n_trees, PosMap pm,
                                                                  double* __restrict__ scores, double* __restrict__ acc) {
    extern __shared__ double dart_lds[];
    if (LDS_VALS) {
        for (uint32_t j = threadIdx.x; j < n_vals; j += DART_BLOCK) dart_lds[j] = vals[j];
        __syncthreads();
    }
    auto value = [&](uint32_t at) { return LDS_VALS ? dart_lds[at] : vals[at]; };
    constexpr uint32_t TILE = DART_BLOCK * DART_DOCS;
    for (uint32_t i0 = blockIdx.x * TILE + threadIdx.x * DART_DOCS; i0 < stride; i0 += gridDim.x * TILE) {
        // (stride is a multiple of 64, hence of DART_DOCS: a lane is inside with all its documents or with none)
        const uint32_t p0 = posmap_at(pm, i0);
        if (p0 == IDX_INVALID) continue;
        const uint16_t* __restrict__ col = leaf + i0;
        double s[DART_DOCS];
#pragma unroll
        for (int j = 0; j < DART_DOCS; j++) s[j] = 0.0;
        constexpr int U = 4;  // trees in flight per lane
        uint32_t k = 0;
        for (; k + U <= n_trees; k += U) {
            uint2 word[U];
            uint32_t base[U];
            double wt[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t t = trees[k + u];
                word[u] = *reinterpret_cast<const uint2*>(col + (size_t)t * stride);
                base[u] = voff[t];
                wt[u] = w[t];
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t l[DART_DOCS] = {word[u].x & 0xFFFFu, word[u].x >> 16, word[u].y & 0xFFFFu, word[u].y >> 16};
#pragma unroll
                for (int j = 0; j < DART_DOCS; j++) {
                    const double prod = wt[u] * value(base[u] + l[j]);
                    s[j] = s[j] + prod;
                }
            }
        }
        for (; k < n_trees; k++) {
            const uint32_t t = trees[k];
            const uint2 word = *reinterpret_cast<const uint2*>(col + (size_t)t * stride);
            const uint32_t base = voff[t];
            const double wt = w[t];
            const uint32_t l[DART_DOCS] = {word.x & 0xFFFFu, word.x >> 16, word.y & 0xFFFFu, word.y >> 16};
#pragma unroll
            for (int j = 0; j < DART_DOCS; j++) {
                const double prod = wt * value(base + l[j]);
                s[j] = s[j] + prod;
            }
        }
#pragma unroll
        for (int j = 0; j < DART_DOCS; j += 2) {
            *reinterpret_cast<double2*>(scores + p0 + j) = make_double2(s[j], s[j + 1]);
            *reinterpret_cast<double2*>(acc + p0 + j) = make_double2(s[j], s[j + 1]);
        }
    }
}
