// Part of device.hip (single translation unit; see that file's header).  The weighted Gram matrix and gradient of the linear
// LambdaRank trainer (DESIGN.md section 18): one pass over the feature tiles on the FP64 matrix units.
// ----------------------------------------------------------------------------------------------
//   H[i][j] = sum_p x_pi * w_p * x_pj   (0 <= i, j < d)        g[i] = sum_p x_pi * lambda_p
// over the documents p of the dataset's (or view's) visited queries; lambda, w: f64 by padded position.
//
// Shape.  A = X^T (features x documents), B = [diag(w) X | lambda] (documents x (d + 1)): column d of B holds lambda_p, so g
// is column d of the product and comes out of the same MFMA stream.  Rows are cut into 16-wide blocks a < nbA = ceil(d / 16),
// columns into blocks b < nbB = ceil((d + 1) / 16); only blocks with a <= b are computed.  Blocks are grouped into panels of
// GRAM_PB = 9 blocks (144 features): a pass (I, J), I <= J, computes the blocks with a in panel I and b in panel J.  At
// d <= 143 there is one pass of at most 45 blocks; wider datasets take further passes (grid dimension y): diagonal ones of
// up to 45 blocks, off-diagonal ones of up to 81.  A pass's blocks are numbered row-major (gram_block_of) and dealt to the four
// waves of a workgroup in contiguous runs of NS = 12 (diagonal) or 21 (off-diagonal); each block's 16 x 16 accumulator is
// four doubles per lane, held in registers for the whole stretch.
//
// A workgroup walks a fixed stretch of 64-document tiles (blockIdx.x * stretch ..; the stretch is a function of the dataset
// alone, gram.inc).  Per tile the 256 threads load the pass's one or two feature panels (nine float4 per thread and panel),
// the tile's w and lambda and the documents' queries into registers -- the loads of tile t + 1 are issued before the
// arithmetic of tile t -- and store them to LDS once:
//   xs[panel][doc][144] f32, row stride 144 floats; ws[doc], ls[doc] f64.
// A position that holds no document of a visited query stores x = 0, w = 0, lambda = 0 and its w and lambda are never loaded:
// a stale NaN there cannot reach the arithmetic.  A k-step covers four documents: lane l reads xs[4 k + l / 16][16 a + l % 16]
// for the A fragment and xs[..][16 b + l % 16] for the B fragment.  The sixteen lanes of a document read consecutive banks and
// the four documents' rows start 144 floats = 16 banks (mod 64, and mod 32) apart, so a fragment read has no bank conflict.
//
// Rounding.  The f32 features widen exactly.  fl(w_p * x_pj) is formed once per fragment in the vector unit (one rounding; the
// same value wherever it is formed again); the MFMA multiplies it by x_pi and adds the four documents of a k-step to the
// accumulator in its own fixed order; lambda_p enters unrounded.  Tiles are added in stretch order, slabs in workgroup order
// (gram_fold_kernel): the result is a function of the dataset and the inputs alone, there are no atomics.
//
// v_mfma_f64_16x16x4_f64 operands: A[i][k] in lane i + 16 k, B[k][j] in lane j + 16 k, D[i][j] in register i / 4 ... see
// gram_acc_row: register r of lane l holds row 4 r + l / 16, column l % 16.

constexpr int GRAM_PB = 9;                    // 16-wide blocks per panel
constexpr int GRAM_PW = GRAM_PB * 16;         // features per panel, and the LDS row stride in floats
constexpr int GRAM_PQ = GRAM_PW / 4;          // float4 columns per panel
constexpr int GRAM_WAVES = 4;
constexpr int GRAM_DIAG_BLOCKS = GRAM_PB * (GRAM_PB + 1) / 2, GRAM_OFF_BLOCKS = GRAM_PB * GRAM_PB;
constexpr int GRAM_DIAG_SLOTS = (GRAM_DIAG_BLOCKS + GRAM_WAVES - 1) / GRAM_WAVES;  // 12 blocks per wave
constexpr int GRAM_OFF_SLOTS = (GRAM_OFF_BLOCKS + GRAM_WAVES - 1) / GRAM_WAVES;    // 21
constexpr int GRAM_FOLD_BATCH = 8;            // slab loads the fold keeps in flight

typedef double gram_acc_t __attribute__((ext_vector_type(4)));

struct GramPass {
    uint32_t I, J, index;  // row panel, column panel, the pass's place in the slab
};

// block t of a pass -> its local row and column block (row-major; a diagonal pass holds the upper triangle only)
__host__ __device__ inline bool gram_block_of(bool diag, uint32_t t, uint32_t* la, uint32_t* lb) {
    if (!diag) {
        *la = t / GRAM_PB, *lb = t % GRAM_PB;
        return t < (uint32_t)GRAM_OFF_BLOCKS;
    }
    uint32_t row = 0;
    while (row < (uint32_t)GRAM_PB && t >= GRAM_PB - row) t -= GRAM_PB - row, row++;
    *la = row, *lb = row + t;
    return row < (uint32_t)GRAM_PB;
}
// the row of a 16 x 16 f64 accumulator that register r of lane l holds (its column is l % 16)
__host__ __device__ inline uint32_t gram_acc_row(uint32_t r, uint32_t lane) { return 4 * r + (lane >> 4); }

struct GramArgs {
    const float4* xb;
    const uint32_t* tiles;  // a view: the tiles that hold its documents (nullptr: every tile)
    uint32_t ntiles, dq, d, nbA, nbB, stretch, slots;
    const uint32_t* qof;           // [np] the query of the document at a position (IDX_INVALID: none of this dataset's)
    const unsigned char* qflags;   // [nq] (nullptr: every query) only flagged queries are visited
    const double *lam, *wt;        // [np]
    double* slab;                  // [pass][workgroup][slots][4][64]
};

template <bool DIAG>
__global__ __launch_bounds__(64 * GRAM_WAVES) void weighted_gram_kernel(GramArgs a, const GramPass* __restrict__ passes) {
    constexpr int NS = DIAG ? GRAM_DIAG_SLOTS : GRAM_OFF_SLOTS;
    constexpr int NP = DIAG ? 1 : 2;  // panels staged
    extern __shared__ double gram_lds[];
    double* ws = gram_lds;                                     // [64]
    double* ls = gram_lds + 64;                                // [64]
    float* xs = reinterpret_cast<float*>(gram_lds + 128);      // [NP][64][GRAM_PW]
    const GramPass ps = passes[blockIdx.y];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t panel[2] = {ps.I, ps.J};

    // this wave's blocks: where their fragments start in a staged row, the global column of lane 0, whether they exist
    uint32_t offA[NS], offB[NS], col0[NS];
    bool valid[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
        uint32_t la = 0, lb = 0;
        const bool in_pass = gram_block_of(DIAG, wave * NS + s, &la, &lb);
        valid[s] = in_pass && ps.I * GRAM_PB + la < a.nbA && ps.J * GRAM_PB + lb < a.nbB;
        offA[s] = 16 * la;
        offB[s] = (DIAG ? 0 : 64 * GRAM_PW) + 16 * lb;
        col0[s] = 16 * (ps.J * GRAM_PB + lb);
    }
    gram_acc_t acc[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = gram_acc_t{0.0, 0.0, 0.0, 0.0};

    const uint32_t t0 = blockIdx.x * a.stretch, t1 = min(t0 + a.stretch, a.ntiles);
    // the tile in flight: thread (wave, lane) holds document `lane`'s float4 columns wave, wave + 4, .. of every panel
    float4 px[NP][GRAM_PQ / GRAM_WAVES];
    double pw = 0.0, pl = 0.0;
    auto fetch = [&](uint32_t ti) {
        const uint32_t tile = a.tiles ? a.tiles[ti] : ti, p = tile * 64 + lane;
        const uint32_t q = a.qof[p];
        const bool live = q != IDX_INVALID && (a.qflags == nullptr || a.qflags[q] != 0);
#pragma unroll
        for (int pn = 0; pn < NP; pn++)
#pragma unroll
            for (int u = 0; u < GRAM_PQ / GRAM_WAVES; u++) {
                const uint32_t j4 = panel[pn] * GRAM_PQ + wave + GRAM_WAVES * u;
                px[pn][u] = (live && j4 < a.dq) ? a.xb[((size_t)tile * a.dq + j4) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        if (wave == 0) {
            pw = live ? a.wt[p] : 0.0;
            pl = live ? a.lam[p] : 0.0;
        }
    };
    if (t0 < t1) fetch(t0);
    for (uint32_t ti = t0; ti < t1; ti++) {
        __syncthreads();  // (the tile before has been read)
#pragma unroll
        for (int pn = 0; pn < NP; pn++)
#pragma unroll
            for (int u = 0; u < GRAM_PQ / GRAM_WAVES; u++)
                *reinterpret_cast<float4*>(xs + ((size_t)pn * 64 + lane) * GRAM_PW + 4 * (wave + GRAM_WAVES * u)) = px[pn][u];
        if (wave == 0) ws[lane] = pw, ls[lane] = pl;
        __syncthreads();
        if (ti + 1 < t1) fetch(ti + 1);
        const uint32_t c = lane & 15;
#pragma unroll 2
        for (uint32_t kk = 0; kk < 16; kk++) {
            const uint32_t doc = 4 * kk + (lane >> 4);
            const double wv = ws[doc], lv = ls[doc];
            const float* row = xs + (size_t)doc * GRAM_PW + c;
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (!valid[s]) continue;
                const double av = (double)row[offA[s]];
                const double xv = (double)row[offB[s]];
                const double prod = wv * xv;  // fl(w_p * x_pj): the one rounding outside the matrix unit
                const double bv = col0[s] + c == a.d ? lv : prod;
                acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[s], 0, 0, 0);
            }
        }
    }
    double* out = a.slab + ((size_t)ps.index * gridDim.x + blockIdx.x) * a.slots * 256;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        if (!valid[s]) continue;
        double* o = out + (size_t)(wave * NS + s) * 256 + lane;
        o[0] = acc[s][0], o[64] = acc[s][1], o[128] = acc[s][2], o[192] = acc[s][3];
    }
}

// H (d x d, both triangles) and g (d) from the slabs: one workgroup per (block, pass), one thread per accumulator entry, the
// workgroups' partial sums added in workgroup order.  Of a diagonal block only the entries on and above the diagonal are read:
// the mirror image is written from them, so H equals its transpose bit for bit.
__global__ __launch_bounds__(256) void gram_fold_kernel(const double* __restrict__ slab, const GramPass* __restrict__ passes, uint32_t G,
                                                        uint32_t slots, uint32_t nbA, uint32_t nbB, uint32_t d, double* __restrict__ H,
                                                        double* __restrict__ g) {
    const GramPass ps = passes[blockIdx.y];
    const bool diag = ps.I == ps.J;
    const uint32_t ns = diag ? GRAM_DIAG_SLOTS : GRAM_OFF_SLOTS, t = blockIdx.x;
    uint32_t la = 0, lb = 0;
    if (t >= GRAM_WAVES * ns || !gram_block_of(diag, t, &la, &lb)) return;
    const uint32_t ba = ps.I * GRAM_PB + la, bb = ps.J * GRAM_PB + lb;
    if (ba >= nbA || bb >= nbB) return;
    const uint32_t e = threadIdx.x, row = 16 * ba + gram_acc_row(e >> 6, e & 63), col = 16 * bb + (e & 15);
    if (row >= d || col > d || (ba == bb && col < row)) return;
    const double* src = slab + ((size_t)ps.index * G * slots + t) * 256 + e;
    const size_t stride = (size_t)slots * 256;
    double sum = 0.0;
    for (uint32_t w0 = 0; w0 < G; w0 += GRAM_FOLD_BATCH) {
        double v[GRAM_FOLD_BATCH];
#pragma unroll
        for (int u = 0; u < GRAM_FOLD_BATCH; u++) v[u] = w0 + u < G ? src[(size_t)(w0 + u) * stride] : 0.0;
#pragma unroll
        for (int u = 0; u < GRAM_FOLD_BATCH; u++)
            if (w0 + u < G) sum = sum + v[u];
    }
    if (col == d) {
        g[row] = sum;
    } else {
        H[(size_t)row * d + col] = sum;
        H[(size_t)col * d + row] = sum;
    }
}

