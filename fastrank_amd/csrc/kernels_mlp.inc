// Part of device.hip (single translation unit; see that file's header).  The one-hidden-layer ReLU net of the NeuralNet model
// and the neural LambdaRank trainer (DESIGN.md section 19): scoring and back-propagation on the FP64 matrix units.
// ----------------------------------------------------------------------------------------------
//   z_pj = b1_j + sum_i x_pi W1_ji     a_pj = z_pj > 0 ? z_pj : 0     s_p = b2 + sum_j a_pj w2_j
//   delta_pj = z_pj > 0 ? fl(lambda_p w2_j) : 0
//   G_W1[j][i] = sum_p delta_pj x_pi   G_b1[j] = sum_p delta_pj   G_w2[j] = sum_p fl(lambda_p a_pj)   G_b2 = sum_p lambda_p
//
// Shape.  Features are cut into panels of MLP_FP = 144 (36 k-steps of four, nine 16-wide blocks), hidden units into panels of
// MLP_HP = 64: wave w of the four waves of a workgroup owns the panel's units 16 w .. 16 w + 15.  A workgroup walks a fixed
// stretch of 64-document tiles (mlp.inc).  A step stages one feature panel of one tile in LDS, once, as
//   xs[doc][MLP_ROW] f32, row stride 148 floats
// (thread (wave, lane) loads document `lane`'s float4 columns wave, wave + 4, ..; the loads of the next step are issued before
// this step's arithmetic).  A position that holds no document of a visited query stages zeros, its lambda is never loaded and
// its score is never written.
//
// First layer.  v_mfma_f64_16x16x4_f64 with A = X (documents x features), B = W1^T (features x units): lane l supplies
// A[i][k] = xs[16 mb + l % 16][4 ks + l / 16] for the four document blocks mb and B[k][j] = W1[unit l % 16][feature 4 ks + l / 16].
// The sixteen documents of a fragment start 148 floats = 20 banks (mod 64) apart -- 20 i mod 64, i < 16, are sixteen different
// multiples of 4 -- and the four features are consecutive: the 64 lanes read 64 different banks.  The B fragments arrive packed in that order (mlp.inc: wf[hp][fp][ks][wave][lane]); with one
// feature panel (d <= 144) a wave's 36 fragments stay in registers for the whole stretch (RES), otherwise they are read from
// the packed array (L2) per step.  The accumulator of block mb starts at b1_j, the k-steps are added with ks ascending, the
// feature panels in ascending order: register r of lane l then holds z of document 16 mb + 4 r + l / 16, unit l % 16.
//
// Output layer (mlp_score_kernel).  t = fl(a w2_j) in the vector unit; the sixteen units of a wave are added by a butterfly
// over the lanes (xor 1, 2, 4, 8: both partners add the same two numbers), the four waves as ((R0 + R1) + R2) + R3 through LDS,
// the hidden panels one after the other onto b2.  Every sum's order is a function of (d, h) alone.
//
// Back-propagation (mlp_backprop_kernel; grid y = hidden panel x feature panel).  z of the pass's hidden panel is recomputed as
// above (over every feature panel: the sign of z never depends on the pass).  delta replaces z in the same registers, and that
// is already the A operand of the second product: G^T = delta^T X has A[i][k] = delta[document 4 kk + l / 16][unit l % 16], which
// is register (mb, r) = (kk / 4, kk % 4) of the same lane.  The delta tile therefore never leaves the registers.  B[k][j] =
// xs[4 kk + l / 16][16 fb + l % 16] (rows 148 floats = 20 banks apart, the lane groups start at banks 0, 20, 40, 60: lanes 52..63
// meet lanes 0..11's banks, a two-way conflict on 12 of 64 lanes, the price of the first layer's conflict-free stride).  A wave accumulates its sixteen units
// against the pass's nine feature blocks (nine accumulators, 144 MFMAs per tile) over the whole stretch; G_b1 and G_w2 are per-lane
// running sums in the vector unit (documents in tile order, (mb, r) ascending), folded over the four lane groups (xor 16, 32)
// at the end; G_b2 is wave 0's per-lane sum folded by a butterfly.  Each workgroup writes one record of MLP_REC doubles;
// mlp_fold_kernel adds the records in workgroup order.  No atomics anywhere.

constexpr int MLP_FP = 144;              // features per panel
constexpr int MLP_KS = MLP_FP / 4;       // k-steps per panel, and float4 columns per panel
constexpr int MLP_FB = MLP_FP / 16;      // 16-wide feature blocks per panel
constexpr int MLP_HP = 64;               // hidden units per panel
constexpr int MLP_ROW = MLP_FP + 4;      // LDS row stride in floats
constexpr int MLP_WAVES = 4;
constexpr int MLP_LOADS = MLP_KS / MLP_WAVES;                 // float4 loads per thread and step
constexpr int MLP_FRAG = MLP_KS * MLP_WAVES * 64;            // doubles of one (hidden panel, feature panel) of packed W1
constexpr int MLP_REC_W1 = MLP_WAVES * MLP_FB * 256;         // a record: [wave][fb][r][lane] ...
constexpr int MLP_REC_B1 = MLP_REC_W1, MLP_REC_W2 = MLP_REC_W1 + MLP_HP, MLP_REC_B2 = MLP_REC_W1 + 2 * MLP_HP;
constexpr int MLP_REC = MLP_REC_W1 + 2 * MLP_HP + 8;         // ... [unit] G_b1, [unit] G_w2, G_b2
constexpr int MLP_FOLD_BATCH = 8;

struct MlpArgs {
    const float4* xb;
    const uint32_t* tiles;  // a view: the tiles that hold its documents (nullptr: every tile)
    uint32_t ntiles, dq, nfp, nhp, stretch;
    const uint32_t* qof;           // [np] the query of the document at a position (IDX_INVALID: none of this dataset's)
    const unsigned char* qflags;   // [nq] (nullptr: every query) only flagged queries are visited
    const double *wf, *b1, *w2;    // packed W1 fragments [nhp][nfp][MLP_FRAG]; b1, w2 zero-padded to nhp * MLP_HP
    double b2;
    const double* lam;             // [np] (back-propagation)
    double* scores;                // [np] (scoring)
    double* slab;                  // [pass][workgroup][MLP_REC] (back-propagation)
};

__device__ __forceinline__ bool mlp_live(const MlpArgs& a, uint32_t p) {
    const uint32_t q = a.qof[p];
    return q != IDX_INVALID && (a.qflags == nullptr || a.qflags[q] != 0);
}
__device__ __forceinline__ void mlp_fetch(const MlpArgs& a, uint32_t tile, uint32_t fp, bool live, uint32_t wave, uint32_t lane,
                                          float4 (&px)[MLP_LOADS]) {
#pragma unroll
    for (int u = 0; u < MLP_LOADS; u++) {
        const uint32_t j4 = fp * MLP_KS + wave + MLP_WAVES * u;
        px[u] = (live && j4 < a.dq) ? a.xb[((size_t)tile * a.dq + j4) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
__device__ __forceinline__ void mlp_stage(float* xs, uint32_t wave, uint32_t lane, const float4 (&px)[MLP_LOADS]) {
#pragma unroll
    for (int u = 0; u < MLP_LOADS; u++) *reinterpret_cast<float4*>(xs + (size_t)lane * MLP_ROW + 4 * (wave + MLP_WAVES * u)) = px[u];
}
// z[mb] += X[16 mb .., this panel] W1^T[this panel, the wave's units]
template <bool RES>
__device__ __forceinline__ void mlp_first_layer(const float* xs, const double (&bw)[MLP_KS], const double* wfrag, uint32_t lane,
                                                gram_acc_t (&z)[4]) {
    const float* row = xs + (size_t)(lane & 15) * MLP_ROW + (lane >> 4);
#pragma unroll
    for (int ks = 0; ks < MLP_KS; ks++) {
        const double bv = RES ? bw[ks] : wfrag[(size_t)ks * MLP_WAVES * 64];
#pragma unroll
        for (int mb = 0; mb < 4; mb++) {
            const double av = (double)row[(size_t)16 * mb * MLP_ROW + 4 * ks];
            z[mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, z[mb], 0, 0, 0);
        }
    }
}

template <bool RES>
__global__ __launch_bounds__(64 * MLP_WAVES) void mlp_score_kernel(MlpArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[64 * MLP_ROW];
    __shared__ double red[MLP_WAVES][64];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    double bw[MLP_KS];
#pragma unroll
    for (int ks = 0; ks < MLP_KS; ks++) bw[ks] = RES ? a.wf[((size_t)ks * MLP_WAVES + wave) * 64 + lane] : 0.0;
    const uint32_t t0 = blockIdx.x * a.stretch, t1 = min(t0 + a.stretch, a.ntiles);
    if (t0 >= t1) return;
    const uint32_t per_tile = a.nhp * a.nfp, nsteps = (t1 - t0) * per_tile;
    float4 px[MLP_LOADS];
    auto fetch = [&](uint32_t s) {
        const uint32_t ti = t0 + s / per_tile, tile = a.tiles ? a.tiles[ti] : ti;
        mlp_fetch(a, tile, s % a.nfp, mlp_live(a, tile * 64 + lane), wave, lane, px);
    };
    fetch(0);
    gram_acc_t z[4];
    double score = 0.0;
    for (uint32_t s = 0; s < nsteps; s++) {
        __syncthreads();  // (the panel before has been read)
        mlp_stage(xs, wave, lane, px);
        __syncthreads();
        if (s + 1 < nsteps) fetch(s + 1);
        const uint32_t fp = s % a.nfp, hp = (s / a.nfp) % a.nhp, unit = hp * MLP_HP + 16 * wave + (lane & 15);
        if (fp == 0) {
            const double bias = a.b1[unit];
#pragma unroll
            for (int mb = 0; mb < 4; mb++) z[mb] = gram_acc_t{bias, bias, bias, bias};
        }
        mlp_first_layer<RES>(xs, bw, a.wf + (size_t)(hp * a.nfp + fp) * MLP_FRAG + wave * 64 + lane, lane, z);
        if (fp + 1 != a.nfp) continue;
        const double w2v = a.w2[unit];
#pragma unroll
        for (int mb = 0; mb < 4; mb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double zz = z[mb][r];
                const double act = zz > 0.0 ? zz : 0.0;
                double t = act * w2v;
                t = t + __shfl_xor(t, 1);
                t = t + __shfl_xor(t, 2);
                t = t + __shfl_xor(t, 4);
                t = t + __shfl_xor(t, 8);
                if ((lane & 15) == 0) red[wave][16 * mb + 4 * r + (lane >> 4)] = t;
            }
        __syncthreads();  // (red is next written two barriers on)
        if (wave == 0) {
            const double panel = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
            score = (hp == 0 ? a.b2 : score) + panel;
            if (hp + 1 == a.nhp) {
                const uint32_t ti = t0 + s / per_tile, p = (a.tiles ? a.tiles[ti] : ti) * 64 + lane;
                if (mlp_live(a, p)) a.scores[p] = score;
            }
        }
    }
}

template <bool RES>
__global__ __launch_bounds__(64 * MLP_WAVES) void mlp_backprop_kernel(MlpArgs a) {
    extern __shared__ __attribute__((aligned(16))) double mlp_lds[];
    double* ls = mlp_lds;                                         // [64] the tile's lambda
    float* xs = reinterpret_cast<float*>(mlp_lds + 64);            // [64][MLP_ROW] the panel of the first layer
    float* xg = RES ? xs : xs + 64 * MLP_ROW;                      // [64][MLP_ROW] the pass's feature panel (RES: the same one)
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t hp = blockIdx.y / a.nfp, gfp = blockIdx.y % a.nfp, unit = hp * MLP_HP + 16 * wave + (lane & 15);
    double bw[MLP_KS];
#pragma unroll
    for (int ks = 0; ks < MLP_KS; ks++) bw[ks] = RES ? a.wf[(size_t)hp * MLP_FRAG + ((size_t)ks * MLP_WAVES + wave) * 64 + lane] : 0.0;
    const double bias = a.b1[unit], w2v = a.w2[unit];
    gram_acc_t g[MLP_FB];
#pragma unroll
    for (int fb = 0; fb < MLP_FB; fb++) g[fb] = gram_acc_t{0.0, 0.0, 0.0, 0.0};
    double gb1 = 0.0, gw2 = 0.0, gb2 = 0.0;

    const uint32_t t0 = blockIdx.x * a.stretch, t1 = min(t0 + a.stretch, a.ntiles);
    const uint32_t nsteps = t0 < t1 ? (t1 - t0) * a.nfp : 0;
    float4 px[MLP_LOADS];
    double pl = 0.0;
    auto fetch = [&](uint32_t s) {
        const uint32_t ti = t0 + s / a.nfp, fp = s % a.nfp, tile = a.tiles ? a.tiles[ti] : ti, p = tile * 64 + lane;
        const bool live = mlp_live(a, p);
        mlp_fetch(a, tile, fp, live, wave, lane, px);
        if (fp == 0 && wave == 0) pl = live ? a.lam[p] : 0.0;
    };
    if (nsteps) fetch(0);
    gram_acc_t z[4];
    for (uint32_t s = 0; s < nsteps; s++) {
        const uint32_t fp = s % a.nfp;
        __syncthreads();  // (the panel before, and with fp == 0 the tile before, has been read)
        mlp_stage(xs, wave, lane, px);
        if (!RES && fp == gfp) mlp_stage(xg, wave, lane, px);
        if (fp == 0 && wave == 0) {
            ls[lane] = pl;
            gb2 = gb2 + pl;
        }
        __syncthreads();
        if (s + 1 < nsteps) fetch(s + 1);
        if (fp == 0) {
#pragma unroll
            for (int mb = 0; mb < 4; mb++) z[mb] = gram_acc_t{bias, bias, bias, bias};
        }
        mlp_first_layer<RES>(xs, bw, a.wf + (size_t)(hp * a.nfp + fp) * MLP_FRAG + wave * 64 + lane, lane, z);
        if (fp + 1 != a.nfp) continue;
        // delta in place of z; the running sums of G_b1 and G_w2
#pragma unroll
        for (int mb = 0; mb < 4; mb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double lv = ls[16 * mb + 4 * r + (lane >> 4)], zz = z[mb][r];
                const bool on = zz > 0.0;
                const double prod = lv * w2v;  // fl(lambda_p * w2_j)
                const double dl = on ? prod : 0.0;
                const double la = lv * (on ? zz : 0.0);  // fl(lambda_p * a_pj)
                gb1 = gb1 + dl;
                gw2 = gw2 + la;
                z[mb][r] = dl;
            }
        // G^T[unit][feature] += delta^T X over the tile's 64 documents
        const float* rowg = xg + (size_t)(lane >> 4) * MLP_ROW + (lane & 15);
#pragma unroll
        for (int kk = 0; kk < 16; kk++) {
            const double av = z[kk >> 2][kk & 3];
#pragma unroll
            for (int fb = 0; fb < MLP_FB; fb++) {
                const double bv = (double)rowg[(size_t)4 * kk * MLP_ROW + 16 * fb];
                g[fb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, g[fb], 0, 0, 0);
            }
        }
    }
    double* rec = a.slab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * MLP_REC;
#pragma unroll
    for (int fb = 0; fb < MLP_FB; fb++) {
        double* o = rec + (size_t)(wave * MLP_FB + fb) * 256 + lane;
        o[0] = g[fb][0], o[64] = g[fb][1], o[128] = g[fb][2], o[192] = g[fb][3];
    }
    gb1 = gb1 + __shfl_xor(gb1, 16), gb1 = gb1 + __shfl_xor(gb1, 32);
    gw2 = gw2 + __shfl_xor(gw2, 16), gw2 = gw2 + __shfl_xor(gw2, 32);
    if (lane < 16) rec[MLP_REC_B1 + 16 * wave + lane] = gb1, rec[MLP_REC_W2 + 16 * wave + lane] = gw2;
    if (wave == 0) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) gb2 = gb2 + __shfl_xor(gb2, m);
        if (lane == 0) rec[MLP_REC_B2] = gb2;
    }
}

// out = [G_W1 (h x d row-major) | G_b1 (h) | G_w2 (h) | G_b2]: one thread per entry, the workgroups' records added in
// workgroup order.
__global__ __launch_bounds__(256) void mlp_fold_kernel(const double* __restrict__ slab, uint32_t G, uint32_t nfp, uint32_t h, uint32_t d,
                                                       double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, nw = (size_t)h * d;
    if (e >= nw + 2 * (size_t)h + 1) return;
    uint32_t pass = 0, off = MLP_REC_B2;
    if (e < nw) {
        const uint32_t j = (uint32_t)(e / d), i = (uint32_t)(e % d), u = j % MLP_HP, f = i % MLP_FP;
        // unit row u % 16 of a 16 x 16 accumulator: register (u % 16) / 4 of the lanes 16 (u % 4) + column
        pass = (j / MLP_HP) * nfp + i / MLP_FP;
        off = ((u / 16) * MLP_FB + f / 16) * 256 + ((u % 16) / 4) * 64 + (u % 4) * 16 + f % 16;
    } else if (e < nw + 2 * (size_t)h) {
        const uint32_t k = (uint32_t)(e - nw), j = k % h;
        pass = (j / MLP_HP) * nfp;
        off = (k < h ? MLP_REC_B1 : MLP_REC_W2) + j % MLP_HP;
    }
    const double* src = slab + (size_t)pass * G * MLP_REC + off;
    double sum = 0.0;
    for (uint32_t w0 = 0; w0 < G; w0 += MLP_FOLD_BATCH) {
        double v[MLP_FOLD_BATCH];
#pragma unroll
        for (int u = 0; u < MLP_FOLD_BATCH; u++) v[u] = w0 + u < G ? src[(size_t)(w0 + u) * MLP_REC] : 0.0;
#pragma unroll
        for (int u = 0; u < MLP_FOLD_BATCH; u++)
            if (w0 + u < G) sum = sum + v[u];
    }
    out[e] = sum;
}

