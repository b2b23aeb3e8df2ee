// Part of device.hip (single translation unit; see that file's header).  Tree-ensemble scoring kernels (config 5 of BASELINE.json).
// (TreeNodeDev, the node record of the L2 walk, is forest_pack.hpp's, with the packers of the layouts described below.)

// Batched tree-ensemble scoring (src/model.rs:64-84,104-112; config 5 of BASELINE.json).
// One thread = one document, one 64-document tile per block.  The block first stages its
// documents' feature rows from the tile into LDS (16-byte loads in, row stride 4*dq+1 dwords so
// lane-strided accesses spread over the banks).  Each lane then walks TI trees at once (TI
// independent pointer chases hide the L1/L2 latency of the 16-byte node records; all lanes walk
// the same trees, so the records stay cache resident) and adds the leaves in tree order:
// out += w_t * leaf_t, unfused (src/model.rs:104-112).
template <bool ROWS_IN_LDS, int TI>
__global__ __launch_bounds__(64) void tree_ensemble_kernel(const float* __restrict__ xb, PosMap pm, uint32_t dq,
                                                           uint32_t d, const TreeNodeDev* __restrict__ nodes,
                                                           const int32_t* __restrict__ roots,
                                                           const double* __restrict__ tw, uint32_t ntrees,
                                                           int raw_single, double* __restrict__ scores) {
    extern __shared__ float rows[];  // [64][4*dq+1]
    const uint32_t tid = threadIdx.x;
    const uint32_t p = posmap_at(pm, blockIdx.x * blockDim.x + tid);  // (whole tiles: always a position)
    const uint32_t rs = dq * 4 + 1;
    if (ROWS_IN_LDS) {
        const float4* xp = (const float4*)xb + (size_t)(p >> 6) * dq * 64 + (p & 63);
        for (uint32_t j4 = 0; j4 < dq; j4++) {
            float4 v = xp[(size_t)j4 * 64];
            float* r = rows + tid * rs + j4 * 4;
            r[0] = v.x;
            r[1] = v.y;
            r[2] = v.z;
            r[3] = v.w;
        }
        __syncthreads();
    }
    const float* myrow = rows + tid * rs;
    double acc = 0.0;
    for (uint32_t t0 = 0; t0 < ntrees; t0 += TI) {
        TreeNodeDev nd[TI];
#pragma unroll
        for (int k = 0; k < TI; k++) nd[k] = nodes[roots[t0 + k < ntrees ? t0 + k : ntrees - 1]];
        bool any_inner = true;
        while (any_inner) {
            any_inner = false;
#pragma unroll
            for (int k = 0; k < TI; k++) {
                if (nd[k].fid >= 0) {
                    float xv;
                    if ((uint32_t)nd[k].fid < d) {
                        xv = ROWS_IN_LDS ? myrow[(uint32_t)nd[k].fid] : xb[xb_index(p, (uint32_t)nd[k].fid, dq)];
                    } else {
                        xv = 0.0f;  // Features::get -> None -> unwrap_or(0.0) (src/model.rs:72-73)
                    }
                    const int32_t next = ((double)xv <= nd[k].split) ? nd[k].lhs : nd[k].lhs + 1;
                    nd[k] = nodes[next];
                    any_inner |= nd[k].fid >= 0;
                }
            }
            any_inner = __any(any_inner);
        }
#pragma unroll
        for (int k = 0; k < TI; k++) {
            if (t0 + k < ntrees) {
                if (raw_single) {
                    acc = nd[k].split;
                } else {
                    double prod = tw[t0 + k] * nd[k].split;
                    acc = acc + prod;
                }
            }
        }
    }
    if (p != IDX_INVALID) scores[p] = acc;
}

// Compact forest for the LDS walk.  The forest is cut into batches that fit the LDS left over by
// the feature columns.  A batch holds H*N trees (H = tree parts per block, N in {1,2,4,8,16} walks
// per thread; see the kernel) as a stream of 8-byte words (padded to a multiple of two):
//   [0, H*N)        per-tree header: lo32 = word index of the root
//   then, per tree, its node words (breadth-first).  The leaf products -- the f64 w_t * leaf (one IEEE
//   multiply, done on the host, bit-identical to doing it per document; the bare leaf for a single-tree
//   model) -- stay in global memory (one gather per walk, L2-resident, < 1 MB per forest): a leaf costs 8
//   bytes of LDS instead of 16, so the LDS left over by the feature columns holds 1.5x as many trees per batch,
//   i.e. twice as many independent walks per thread (measured at the 30K shape, 192 x 4 blocks: 8 walks per
//   thread with the gather 5.6 ms, 4 walks with the products in LDS 6.2 ms).
// Node word = { lo32: f32 thr; hi32: u24 feature byte offset | u8 rel << 24 }, children adjacent,
// left child at self + rel, right child at self + rel + 1:
//   internal: thr = largest f32 <= split, so for every f32 x (f64(x) <= split) <=> (x <= thr)
//             (src/model.rs:75-79); byte offset = slot * DOCS * 4 (features are slot-major in LDS).
//             A feature the dataset does not have reads 0.0 (Features::get -> None ->
//             unwrap_or(0.0), src/model.rs:72-73): such nodes use the padding slot, which holds 0.0.
//   leaf:     the padding slot (x = 0.0), rel = 0 and thr's bits = the index of the leaf's product in the
//             forest's global product array (a non-negative float, so 0.0 <= thr and the walk stays put).
// One step of a walk is therefore branch-free: cur += rel + (x <= thr ? 0 : 1).
// Batches that cannot be filled with real trees are padded with one-leaf trees whose product is
// +0.0, the identity for a sum that starts at +0.0.
typedef uint32_t fr_u32x4 __attribute__((ext_vector_type(4)));  // plain 16-byte vector (stays in registers)

// N concurrent walks (trees t0 .. t0+N-1 of the LDS batch) for one document; prod[k] = w_t * leaf_t.  `mycol` = LDS byte address of the document's feature
// column; a node's slot field is the byte offset of its feature inside that column.
template <int N>
__device__ __forceinline__ void tree_walk_group(const uint64_t* trees, const double* __restrict__ leafprod, uint32_t mycol,
                                                uint32_t t0, uint32_t levels, double (&prod)[N]) {
    uint32_t cur[N];
#pragma unroll
    for (int k = 0; k < N; k++) cur[k] = (uint32_t)trees[t0 + k];
    for (uint32_t lv = 0; lv < levels; lv++) {
        uint64_t word[N];
#pragma unroll
        for (int k = 0; k < N; k++) word[k] = trees[cur[k]];
        // keep the three phases apart in the schedule: all N node reads in flight together, then all N
        // feature reads (one exposed LDS latency per phase instead of one per small cluster of walks)
        __builtin_amdgcn_sched_barrier(0);
        float xv[N];
#pragma unroll
        for (int k = 0; k < N; k++) {
            // LDS byte address of the feature: column base + low 24 bits of hi32, in one v_mad_u32_u24
            uint32_t addr;
            asm("v_mad_u32_u24 %0, %1, 1, %2" : "=v"(addr) : "v"((uint32_t)(word[k] >> 32)), "v"(mycol));
            xv[k] = *(const __attribute__((address_space(3))) float*)(uintptr_t)addr;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < N; k++) {
            // cur += rel + (x <= thr ? 0 : 1): the compare's carry and byte 3 of hi32 in one SDWA add
// (no wait state is needed between the compare and the SDWA add that takes VCC as its carry: the 13 tree parity
// tests and a 20 000-document x 500-tree bit-exact check pass without one, 3 % faster; -DTREE_WITH_NOP restores it)
#ifdef TREE_WITH_NOP
#define TREE_NOP "s_nop 1\n\t"
#else
#define TREE_NOP ""
#endif
            asm("v_cmp_nle_f32 vcc, %2, %3\n\t" TREE_NOP
                "v_addc_co_u32_sdwa %0, vcc, %1, %4, vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3"
                : "=v"(cur[k])
                : "v"(cur[k]), "v"(xv[k]), "v"((uint32_t)word[k]), "v"((uint32_t)(word[k] >> 32))
                : "vcc");
        }
    }
#pragma unroll
    for (int k = 0; k < N; k++) prod[k] = leafprod[(uint32_t)trees[cur[k]]];
}

// One part's share of a batch: walk N trees, then add the N products to the document's running sum
// when it is this part's turn (parts take turns in tree order; H == 1 keeps the sum in `acc`).
template <int N, int H>
__device__ __forceinline__ void tree_batch_part(const uint64_t* trees, const double* __restrict__ leafprod, uint32_t mycol,
                                                uint32_t part, uint32_t levels, int raw_single, double* runslot, double& acc) {
    double prod[N];
    tree_walk_group<N>(trees, leafprod, mycol, part * N, levels, prod);
    if (H == 1) {
        if (raw_single) {
            acc = prod[0];
        } else {
#pragma unroll
            for (int k = 0; k < N; k++) acc = acc + prod[k];
        }
    } else {
#pragma unroll
        for (int h = 0; h < H; h++) {
            if (part == (uint32_t)h) {
                double a = *runslot;
#pragma unroll
                for (int k = 0; k < N; k++) a = a + prod[k];
                *runslot = a;
            }
            if (h + 1 < H) __syncthreads();
        }
    }
}

// One prefetch slot of the forest stream: PF 16-byte words per thread, in registers.
template <int PF>
struct TreePrefetch {
    fr_u32x4 v[PF];
    uint32_t n16;
    __device__ __forceinline__ void fetch(const fr_u32x4* __restrict__ forest, const uint32_t* __restrict__ batch_desc,
                                          uint32_t b, uint32_t tid, uint32_t bs) {
        const uint32_t base = batch_desc[b * 4];
        n16 = batch_desc[b * 4 + 4] - base;
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const uint32_t idx = tid + (uint32_t)i * bs;
            v[i] = forest[base + (idx < n16 ? idx : 0u)];
        }
    }
    __device__ __forceinline__ void commit(fr_u32x4* trees16, uint32_t tid, uint32_t bs) const {
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const uint32_t idx = tid + (uint32_t)i * bs;
            if (idx < n16) trees16[idx] = v[i];
        }
    }
};

// Batched tree-ensemble scoring, LDS-resident trees (the fast path of config 5).
// A block owns DOCS documents (whole 64-document tiles): their features are staged in LDS
// slot-major ([4*dq+1][DOCS]; the extra slot is the 0.0 padding slot), so whatever slot a lane
// reads it hits bank lane % 64 and divergent walks never conflict on feature reads.  The forest
// streams through the rest of the LDS batch by batch; two batches are in flight in registers (PF
// 16-byte words per thread each), so the L2/HBM round trip of a batch hides behind the walk of the
// previous one.  The H thread groups ("parts") of a block all see the same documents and split a
// batch's trees H ways: fewer documents per block leave room for larger batches (the per-batch
// barriers and hand-over are the fixed cost) while the CU keeps DOCS*H/64 waves.
// Every thread walks its N trees concurrently, `levels` steps each, and keeps the N products
// w_t * leaf_t; the parts then add their products to the document's running sum one part after
// the other (through an LDS slot per document), so the sum is formed in tree order:
// out += w_t * leaf_t, unfused (src/model.rs:104-112).
template <int DOCS, int H, int PF>
__global__ __launch_bounds__(DOCS * H) void tree_ensemble_lds_kernel(
    const float* __restrict__ xb, PosMap pm, uint32_t dq, const fr_u32x4* __restrict__ forest,
    const uint32_t* __restrict__ batch_desc /*[nbatch+1][4]: offset (16-byte units), N, levels, 0*/,
    uint32_t nbatch, int raw_single, const double* __restrict__ leafprod, double* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw8[];
    constexpr uint32_t bs = DOCS * H, docs = DOCS;
    float* cols = (float*)lds_raw8;                                        // [4*dq+1][DOCS]
    const uint32_t cols_bytes = ((dq * 4 + 1) * docs * 4 + 15u) & ~15u;
    double* run = (double*)(lds_raw8 + cols_bytes);                        // [DOCS] running sums (H > 1)
    uint64_t* trees = (uint64_t*)(run + (H > 1 ? docs : 0));               // one batch
    fr_u32x4* trees16 = (fr_u32x4*)trees;
    const uint32_t tid = threadIdx.x;
    const uint32_t doc = tid % docs, part = tid / docs;
    const uint32_t p = posmap_at(pm, blockIdx.x * docs + doc);  // (IDX_INVALID past the last tile: the last block may be ragged)
    const uint32_t pc = p != IDX_INVALID ? p : posmap_at(pm, 0u);
    TreePrefetch<PF> pa, pb;
    pa.fetch(forest, batch_desc, 0, tid, bs);
    if (nbatch > 1) pb.fetch(forest, batch_desc, 1, tid, bs);
    {
        // part h stages the float4 groups j4 = h, h + H, ...
        const float4* xp = (const float4*)xb + (size_t)(pc >> 6) * dq * 64 + (pc & 63);
        float* c = cols + doc;
        for (uint32_t j4 = part; j4 < dq; j4 += H) {
            float4 v = xp[(size_t)j4 * 64];
            c[(j4 * 4 + 0) * docs] = v.x;
            c[(j4 * 4 + 1) * docs] = v.y;
            c[(j4 * 4 + 2) * docs] = v.z;
            c[(j4 * 4 + 3) * docs] = v.w;
        }
        if (part == 0) {
            c[dq * 4 * docs] = 0.0f;
            if (H > 1) run[doc] = 0.0;
        }
    }
    const uint32_t mycol = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)(cols + doc);
    double acc = 0.0;  // H == 1: the running sum lives here
#define FR_TREE_BATCH(SLOT, B)                                                                                  \
    if ((B) < nbatch) {                                                                                         \
        const uint32_t n = batch_desc[(B) * 4 + 1], levels = batch_desc[(B) * 4 + 2];                           \
        __syncthreads(); /* previous batch fully consumed, its sums published */                                \
        SLOT.commit(trees16, tid, bs);                                                                          \
        __syncthreads(); /* this batch (and, first time round, the feature columns) visible */                  \
        if ((B) + 2 < nbatch) SLOT.fetch(forest, batch_desc, (B) + 2, tid, bs);                                 \
        if (n == 16) tree_batch_part<16, H>(trees, leafprod, mycol, part, levels, raw_single, run + doc, acc);  \
        else if (n == 8) tree_batch_part<8, H>(trees, leafprod, mycol, part, levels, raw_single, run + doc, acc); \
        else if (n == 4) tree_batch_part<4, H>(trees, leafprod, mycol, part, levels, raw_single, run + doc, acc); \
        else if (n == 2) tree_batch_part<2, H>(trees, leafprod, mycol, part, levels, raw_single, run + doc, acc); \
        else tree_batch_part<1, H>(trees, leafprod, mycol, part, levels, raw_single, run + doc, acc);           \
    }
    for (uint32_t b = 0; b < nbatch; b += 2) {
        FR_TREE_BATCH(pa, b)
        FR_TREE_BATCH(pb, b + 1)
    }
#undef FR_TREE_BATCH
    if (H > 1) {
        __syncthreads();
        acc = run[doc];
    }
    if (part == 0 && p != IDX_INVALID) scores[p] = acc;
}
