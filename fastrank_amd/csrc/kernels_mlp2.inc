// Part of device.hip (single translation unit; see that file's header).  The NeuralNet model with a second hidden layer
// (DESIGN.md section 19, "Two hidden layers"): scoring chains three tile products on the FP64 matrix units, back-propagation five.
// ----------------------------------------------------------------------------------------------
//   z1_pj = b1_j + sum_i x_pi W1_ji        a1_pj = z1_pj > 0 ? z1_pj : 0
//   z2_pk = c_k  + sum_j a1_pj W2_kj       a2_pk = z2_pk > 0 ? z2_pk : 0        s_p = b_out + sum_k fl(a2_pk w3_k)
//   d2_pk = z2_pk > 0 ? fl(lambda_p w3_k) : 0          G_w3[k] = sum_p fl(lambda_p a2_pk)     G_bout = sum_p lambda_p
//   G_W2[k][j] = sum_p d2_pk a1_pj         G_c[k] = sum_p d2_pk
//   e_pj = sum_k d2_pk W2_kj               d1_pj = z1_pj > 0 ? e_pj : 0
//   G_W1[j][i] = sum_p d1_pj x_pi          G_b1[j] = sum_p d1_pj
//
// The first layer is kernels_mlp.inc's as it stands: the staging of xs[64][148], the W1 fragments (resident with one feature
// panel and one hidden panel), four waves that own sixteen units each of a 64-unit hidden panel, z1 of (document 16 mb + 4 r +
// l / 16, unit l % 16) in register r of accumulator mb.  h2 <= 64: the second layer is one panel, wave w owns its units 16 w ..
// 16 w + 15 and holds their z2 for the tile's 64 documents in four accumulators, the same layout one layer up.
//
// Second layer.  z2 contracts over first-layer units, which the four waves hold sixteen each, in a layout that is neither
// fragment of such a product.  So a1 of one hidden panel goes through LDS once, as
//   as[doc][MLP2_ROW] f64, row stride 66 doubles,
// and after a barrier every wave reads A[i][k] = as[16 mb + l % 16][4 kk + l / 16] against B[k][j] = W2[unit 16 w + l % 16][first-
// layer unit 64 hp + 4 kk + l / 16], packed on the host in that order (w2f[hp][kk][wave][lane]).  An 8-byte LDS read is served
// half a wave at a time over 32 double-wide banks: lanes 0..31 read rows l % 16 at columns c, c + 1, and 66 i + c mod 32 =
// 2 i + c runs through 32 different values for i < 16, c < 2 (lanes 32..63 likewise, two columns on): no conflict.  (A stride
// of 64 would put all sixteen rows on one bank.)  The writes, and back-propagation's B reads along a row, touch two rows of
// sixteen consecutive columns per half-wave, 0..15 and 2..17 mod 32: fourteen banks twice, on a quarter as many accesses.
// 16 k-steps x 4 document blocks = 64 MFMAs per wave and hidden panel; the accumulators start at c_k and stay in registers
// across the hidden panels, which come in ascending order.  k-steps past the model's last first-layer unit, and waves whose
// sixteen second-layer units the model does not have, are skipped (both wave-uniform).
//
// Output layer: kernels_mlp.inc's over a2 -- t = fl(a2 w3_k), butterfly over the sixteen lanes, ((R0 + R1) + R2) + R3 onto b_out.
//
// Back-propagation (grid y = hidden panel x feature panel, as for one layer).  Per tile the workgroup walks every hidden panel
// as the score kernel does, so z2 has the bits scoring saw in every pass, and keeps z1 of its own panel.  d2 replaces z2 in
// registers (G_w3, G_c per-lane running sums).  G_W2^T[unit k][unit j] = sum_p d2_pk a1_pj contracts over documents: its A operand
// is register (kk / 4, kk % 4) of the same lane, as in the one-layer kernel, B[k][j] = as[4 kk + l / 16][16 ub + l % 16] is a1 of the
// own panel, put back into LDS from the kept z1 when another panel came after it; four accumulators for the stretch (feature
// panel 0's pass only: the others would repeat it).  Then d2 goes through the same buffer and e = d2 W2 is the second layer's
// product with B[k][j] = W2[unit 4 kk + l / 16][own unit 16 w + l % 16] (w2b[hp][kk][wave][lane], resident), which lands in z1's
// layout: d1 is a select, and the one-layer kernel's G_W1 product and G_b1 sums follow.  One record of MLP2_REC doubles per
// workgroup and pass; mlp2_fold_kernel adds them in workgroup order.  No atomics anywhere.

constexpr int MLP2_ROW = 66;                                   // LDS row stride of the a1 / d2 tile in doubles
constexpr int MLP2_KK = MLP_HP / 4;                            // k-steps of a product that contracts over 64 units
constexpr int MLP2_FRAG = MLP2_KK * MLP_WAVES * 64;            // doubles of one hidden panel of packed W2, either order
constexpr int MLP2_REC_W2 = MLP_REC_W1;                        // a record: the one-layer G_W1 block, [wave][ub][r][lane] G_W2^T, ...
constexpr int MLP2_REC_B1 = MLP2_REC_W2 + MLP_WAVES * 4 * 256, MLP2_REC_C = MLP2_REC_B1 + MLP_HP, MLP2_REC_W3 = MLP2_REC_C + MLP_HP;
constexpr int MLP2_REC_BOUT = MLP2_REC_W3 + MLP_HP;            // ... [unit] G_b1, [unit] G_c, [unit] G_w3, G_bout
constexpr int MLP2_REC = MLP2_REC_BOUT + 8;

struct Mlp2Args {
    MlpArgs m;                     // the first layer; m.w2 = w3 zero-padded to 64, m.b2 = b_out
    const double *w2f, *w2b, *c;   // packed W2 [nhp][MLP2_FRAG] for z2 and for e; c zero-padded to 64
    uint32_t h, h2;
};

// as[doc][unit of the panel] <- v (RELU: v > 0 ? v : 0), from the accumulators' layout
template <bool RELU>
__device__ __forceinline__ void mlp2_put(double* as, uint32_t wave, uint32_t lane, const gram_acc_t (&v)[4]) {
    double* o = as + (size_t)(lane >> 4) * MLP2_ROW + 16 * wave + (lane & 15);
#pragma unroll
    for (int mb = 0; mb < 4; mb++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double x = v[mb][r];
            o[(size_t)(16 * mb + 4 * r) * MLP2_ROW] = RELU ? (x > 0.0 ? x : 0.0) : x;
        }
}
// acc[mb] += T[16 mb .., 4 kk ..] F[4 kk .., the wave's sixteen] over the k-steps below nk, ascending
__device__ __forceinline__ void mlp2_tile_product(const double* as, const double (&bf)[MLP2_KK], uint32_t nk, uint32_t lane, gram_acc_t (&acc)[4]) {
    const double* row = as + (size_t)(lane & 15) * MLP2_ROW + (lane >> 4);
#pragma unroll
    for (int kk = 0; kk < MLP2_KK; kk++) {
        if ((uint32_t)kk < nk) {
#pragma unroll
            for (int mb = 0; mb < 4; mb++)
                acc[mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[(size_t)16 * mb * MLP2_ROW + 4 * kk], bf[kk], acc[mb], 0, 0, 0);
        }
    }
}
__device__ __forceinline__ void mlp2_load_frag(const double* frag, uint32_t wave, uint32_t lane, double (&bf)[MLP2_KK]) {
#pragma unroll
    for (int kk = 0; kk < MLP2_KK; kk++) bf[kk] = frag[((size_t)kk * MLP_WAVES + wave) * 64 + lane];
}
// k-steps that hold a first-layer unit of hidden panel hp
__device__ __forceinline__ uint32_t mlp2_ksteps(uint32_t h, uint32_t hp) { return (min(h - hp * MLP_HP, (uint32_t)MLP_HP) + 3) / 4; }

// dynamic LDS: as[64][MLP2_ROW] f64 | red[MLP_WAVES][64] f64 | xs[64][MLP_ROW] f32
template <bool RES>
__global__ __launch_bounds__(64 * MLP_WAVES) void mlp2_score_kernel(Mlp2Args a2) {
    extern __shared__ __attribute__((aligned(16))) double mlp2_lds[];
    const MlpArgs& a = a2.m;
    double* as = mlp2_lds;
    double* red = as + 64 * MLP2_ROW;
    float* xs = reinterpret_cast<float*>(red + MLP_WAVES * 64);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    double bw[MLP_KS], bf[MLP2_KK];
#pragma unroll
    for (int ks = 0; ks < MLP_KS; ks++) bw[ks] = RES ? a.wf[((size_t)ks * MLP_WAVES + wave) * 64 + lane] : 0.0;
    if (RES) mlp2_load_frag(a2.w2f, wave, lane, bf);
    const bool own2 = 16 * wave < a2.h2;  // the model has some of the wave's second-layer units
    const double cv = a2.c[16 * wave + (lane & 15)], w3v = a.w2[16 * wave + (lane & 15)];
    const uint32_t t0 = blockIdx.x * a.stretch, t1 = min(t0 + a.stretch, a.ntiles);
    if (t0 >= t1) return;
    const uint32_t per_tile = a.nhp * a.nfp, nsteps = (t1 - t0) * per_tile;
    float4 px[MLP_LOADS];
    auto fetch = [&](uint32_t s) {
        const uint32_t ti = t0 + s / per_tile, tile = a.tiles ? a.tiles[ti] : ti;
        mlp_fetch(a, tile, s % a.nfp, mlp_live(a, tile * 64 + lane), wave, lane, px);
    };
    fetch(0);
    gram_acc_t z[4], z2[4];
    for (uint32_t s = 0; s < nsteps; s++) {
        __syncthreads();  // (the panel before, and the a1 tile before, have been read)
        mlp_stage(xs, wave, lane, px);
        __syncthreads();
        if (s + 1 < nsteps) fetch(s + 1);
        const uint32_t fp = s % a.nfp, hp = (s / a.nfp) % a.nhp;
        if (fp == 0) {
            const double bias = a.b1[hp * MLP_HP + 16 * wave + (lane & 15)];
#pragma unroll
            for (int mb = 0; mb < 4; mb++) z[mb] = gram_acc_t{bias, bias, bias, bias};
        }
        mlp_first_layer<RES>(xs, bw, a.wf + (size_t)(hp * a.nfp + fp) * MLP_FRAG + wave * 64 + lane, lane, z);
        if (fp + 1 != a.nfp) continue;
        mlp2_put<true>(as, wave, lane, z);
        if (!RES && own2) mlp2_load_frag(a2.w2f + (size_t)hp * MLP2_FRAG, wave, lane, bf);
        __syncthreads();
        if (hp == 0) {
#pragma unroll
            for (int mb = 0; mb < 4; mb++) z2[mb] = gram_acc_t{cv, cv, cv, cv};
        }
        if (own2) mlp2_tile_product(as, bf, mlp2_ksteps(a2.h, hp), lane, z2);
        if (hp + 1 != a.nhp) continue;
#pragma unroll
        for (int mb = 0; mb < 4; mb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double zz = z2[mb][r];
                const double act = zz > 0.0 ? zz : 0.0;
                double t = act * w3v;  // fl(a2 * w3_k)
                t = t + __shfl_xor(t, 1);
                t = t + __shfl_xor(t, 2);
                t = t + __shfl_xor(t, 4);
                t = t + __shfl_xor(t, 8);
                if ((lane & 15) == 0) red[wave * 64 + 16 * mb + 4 * r + (lane >> 4)] = t;
            }
        __syncthreads();  // (red is next written two barriers on)
        if (wave == 0) {
            const double sum = ((red[lane] + red[64 + lane]) + red[128 + lane]) + red[192 + lane];
            const uint32_t ti = t0 + s / per_tile, p = (a.tiles ? a.tiles[ti] : ti) * 64 + lane;
            if (mlp_live(a, p)) a.scores[p] = a.b2 + sum;
        }
    }
}

// dynamic LDS: as[64][MLP2_ROW] f64 | ls[64] f64 | xs[64][MLP_ROW] f32 | with several feature panels xg[64][MLP_ROW] f32
// (W1's fragments are read per step: resident next to the thirteen accumulators, the kept z1 and W2's, they spilled)
__global__ __launch_bounds__(64 * MLP_WAVES) void mlp2_backprop_kernel(Mlp2Args a2) {
    extern __shared__ __attribute__((aligned(16))) double mlp2_lds[];
    const MlpArgs& a = a2.m;
    double* as = mlp2_lds;                                        // the a1 tile of a hidden panel, then the d2 tile
    double* ls = as + 64 * MLP2_ROW;                              // the tile's lambda
    float* xs = reinterpret_cast<float*>(ls + 64);                // the panel of the first layer
    float* xg = a.nfp == 1 ? xs : xs + 64 * MLP_ROW;              // the pass's feature panel
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t hp = blockIdx.y / a.nfp, gfp = blockIdx.y % a.nfp;
    const double bw[MLP_KS] = {};  // (not read)
    double bf[MLP2_KK], bb[MLP2_KK];
    mlp2_load_frag(a2.w2b + (size_t)hp * MLP2_FRAG, wave, lane, bb);
    const bool own1 = hp * MLP_HP + 16 * wave < a2.h, own2 = 16 * wave < a2.h2;  // the model has some of the wave's units
    const uint32_t nk2 = (a2.h2 + 3) / 4;
    const double cv = a2.c[16 * wave + (lane & 15)], w3v = a.w2[16 * wave + (lane & 15)];
    gram_acc_t g[MLP_FB], gw[4];
#pragma unroll
    for (int fb = 0; fb < MLP_FB; fb++) g[fb] = gram_acc_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ub = 0; ub < 4; ub++) gw[ub] = gram_acc_t{0.0, 0.0, 0.0, 0.0};
    double gb1 = 0.0, gc = 0.0, gw3 = 0.0, gbo = 0.0;

    const uint32_t t0 = blockIdx.x * a.stretch, t1 = min(t0 + a.stretch, a.ntiles);
    const uint32_t per_tile = a.nhp * a.nfp, nsteps = t0 < t1 ? (t1 - t0) * per_tile : 0;
    float4 px[MLP_LOADS];
    double pl = 0.0;
    auto fetch = [&](uint32_t s) {
        const uint32_t ti = t0 + s / per_tile, tile = a.tiles ? a.tiles[ti] : ti, p = tile * 64 + lane;
        const bool live = mlp_live(a, p);
        mlp_fetch(a, tile, s % a.nfp, live, wave, lane, px);
        if (s % per_tile == 0 && wave == 0) pl = live ? a.lam[p] : 0.0;
    };
    if (nsteps) fetch(0);
    gram_acc_t z[4], z2[4], zk[4];
    for (uint32_t s = 0; s < nsteps; s++) {
        const uint32_t fp = s % a.nfp, php = (s / a.nfp) % a.nhp;
        __syncthreads();  // (the panel before and the tile in `as` have been read; with s % per_tile == 0 so has the tile before)
        mlp_stage(xs, wave, lane, px);
        if (a.nfp != 1 && fp == gfp) mlp_stage(xg, wave, lane, px);
        if (s % per_tile == 0 && wave == 0) {
            ls[lane] = pl;
            gbo = gbo + pl;
        }
        __syncthreads();
        if (s + 1 < nsteps) fetch(s + 1);
        if (fp == 0) {
            const double bias = a.b1[php * MLP_HP + 16 * wave + (lane & 15)];
#pragma unroll
            for (int mb = 0; mb < 4; mb++) z[mb] = gram_acc_t{bias, bias, bias, bias};
        }
        mlp_first_layer<false>(xs, bw, a.wf + (size_t)(php * a.nfp + fp) * MLP_FRAG + wave * 64 + lane, lane, z);
        if (fp + 1 != a.nfp) continue;
        // z2 += a1 W2^T of this hidden panel; z1 of the pass's own panel is kept
        if (php == hp) {
#pragma unroll
            for (int mb = 0; mb < 4; mb++) zk[mb] = z[mb];
        }
        mlp2_put<true>(as, wave, lane, z);
        if (own2) mlp2_load_frag(a2.w2f + (size_t)php * MLP2_FRAG, wave, lane, bf);
        __syncthreads();
        if (php == 0) {
#pragma unroll
            for (int mb = 0; mb < 4; mb++) z2[mb] = gram_acc_t{cv, cv, cv, cv};
        }
        if (own2) mlp2_tile_product(as, bf, mlp2_ksteps(a2.h, php), lane, z2);
        if (php + 1 != a.nhp) continue;
        // d2 in place of z2; the running sums of G_c and G_w3
#pragma unroll
        for (int mb = 0; mb < 4; mb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double lv = ls[16 * mb + 4 * r + (lane >> 4)], zz = z2[mb][r];
                const bool on = zz > 0.0;
                const double prod = lv * w3v;  // fl(lambda_p * w3_k)
                const double dl = on ? prod : 0.0;
                const double la = lv * (on ? zz : 0.0);  // fl(lambda_p * a2_pk)
                gc = gc + dl;
                gw3 = gw3 + la;
                z2[mb][r] = dl;
            }
        if (hp + 1 != a.nhp) {  // `as` holds the last panel's a1: the own panel's again, from the kept z1
            __syncthreads();
            mlp2_put<true>(as, wave, lane, zk);
        }
        __syncthreads();
        // G_W2^T[the wave's units k][the own panel's units j] += d2^T a1 over the tile's 64 documents
        if (gfp == 0 && own2) {
            const double* rowa = as + (size_t)(lane >> 4) * MLP2_ROW + (lane & 15);
#pragma unroll
            for (int kk = 0; kk < 16; kk++) {
                const double av = z2[kk >> 2][kk & 3];
#pragma unroll
                for (int ub = 0; ub < 4; ub++) gw[ub] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, rowa[(size_t)4 * kk * MLP2_ROW + 16 * ub], gw[ub], 0, 0, 0);
            }
        }
        __syncthreads();  // (a1 has been read)
        mlp2_put<false>(as, wave, lane, z2);
        __syncthreads();
        if (!own1) continue;
        // e = d2 W2 for the wave's own first-layer units, d1 in place of z; the running sum of G_b1
#pragma unroll
        for (int mb = 0; mb < 4; mb++) z[mb] = gram_acc_t{0.0, 0.0, 0.0, 0.0};
        mlp2_tile_product(as, bb, nk2, lane, z);
#pragma unroll
        for (int mb = 0; mb < 4; mb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double dl = zk[mb][r] > 0.0 ? z[mb][r] : 0.0;
                gb1 = gb1 + dl;
                z[mb][r] = dl;
            }
        // G_W1^T[unit][feature] += d1^T X over the tile's 64 documents
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
    double* rec = a.slab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * MLP2_REC;
#pragma unroll
    for (int fb = 0; fb < MLP_FB; fb++) {
        double* o = rec + (size_t)(wave * MLP_FB + fb) * 256 + lane;
        o[0] = g[fb][0], o[64] = g[fb][1], o[128] = g[fb][2], o[192] = g[fb][3];
    }
#pragma unroll
    for (int ub = 0; ub < 4; ub++) {
        double* o = rec + MLP2_REC_W2 + (size_t)(wave * 4 + ub) * 256 + lane;
        o[0] = gw[ub][0], o[64] = gw[ub][1], o[128] = gw[ub][2], o[192] = gw[ub][3];
    }
    gb1 = gb1 + __shfl_xor(gb1, 16), gb1 = gb1 + __shfl_xor(gb1, 32);
    gc = gc + __shfl_xor(gc, 16), gc = gc + __shfl_xor(gc, 32);
    gw3 = gw3 + __shfl_xor(gw3, 16), gw3 = gw3 + __shfl_xor(gw3, 32);
    if (lane < 16) rec[MLP2_REC_B1 + 16 * wave + lane] = gb1, rec[MLP2_REC_C + 16 * wave + lane] = gc, rec[MLP2_REC_W3 + 16 * wave + lane] = gw3;
    if (wave == 0) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) gbo = gbo + __shfl_xor(gbo, m);
        if (lane == 0) rec[MLP2_REC_BOUT] = gbo;
    }
}

// out = [G_W1 (h x d row-major) | G_b1 (h) | G_W2 (h2 x h row-major) | G_c (h2) | G_w3 (h2) | G_bout], the trainer's parameter
// order: one thread per entry, the workgroups' records added in workgroup order.  G_W1 comes from the pass of its (hidden
// panel, feature panel), G_b1 and G_W2 from feature panel 0's pass of their hidden panel, the rest from pass 0.
__global__ __launch_bounds__(256) void mlp2_fold_kernel(const double* __restrict__ slab, uint32_t G, uint32_t nfp, uint32_t h, uint32_t h2, uint32_t d,
                                                        double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, nw = (size_t)h * d, nw2 = (size_t)h2 * h;
    if (e >= nw + h + nw2 + 2 * (size_t)h2 + 1) return;
    uint32_t pass = 0, off = MLP2_REC_BOUT;
    if (e < nw) {
        const uint32_t j = (uint32_t)(e / d), i = (uint32_t)(e % d), u = j % MLP_HP, f = i % MLP_FP;
        pass = (j / MLP_HP) * nfp + i / MLP_FP;
        off = ((u / 16) * MLP_FB + f / 16) * 256 + ((u % 16) / 4) * 64 + (u % 4) * 16 + f % 16;
    } else if (e < nw + h) {
        const uint32_t j = (uint32_t)(e - nw);
        pass = (j / MLP_HP) * nfp;
        off = MLP2_REC_B1 + j % MLP_HP;
    } else if (e < nw + h + nw2) {
        // row k % 16 of the 16 x 16 accumulator (k / 16, (j % 64) / 16): register (k % 16) / 4 of the lanes 16 (k % 4) + column
        const uint32_t k = (uint32_t)((e - nw - h) / h), j = (uint32_t)((e - nw - h) % h), u = j % MLP_HP;
        pass = (j / MLP_HP) * nfp;
        off = MLP2_REC_W2 + ((k / 16) * 4 + u / 16) * 256 + ((k % 16) / 4) * 64 + (k % 4) * 16 + u % 16;
    } else if (e < nw + h + nw2 + 2 * (size_t)h2) {
        const uint32_t k = (uint32_t)(e - nw - h - nw2);
        off = k < h2 ? MLP2_REC_C + k : MLP2_REC_W3 + (k - h2);
    }
    const double* src = slab + (size_t)pass * G * MLP2_REC + off;
    double sum = 0.0;
    for (uint32_t w0 = 0; w0 < G; w0 += MLP_FOLD_BATCH) {
        double v[MLP_FOLD_BATCH];
#pragma unroll
        for (int u = 0; u < MLP_FOLD_BATCH; u++) v[u] = w0 + u < G ? src[(size_t)(w0 + u) * MLP2_REC] : 0.0;
#pragma unroll
        for (int u = 0; u < MLP_FOLD_BATCH; u++)
            if (w0 + u < G) sum = sum + v[u];
    }
    out[e] = sum;
}
