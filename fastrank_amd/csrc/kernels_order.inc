// Part of device.hip (single translation unit; see that file's header).  The visiting-order tables of the resident NDCG@k
// verify kernel (kernels_verify.inc, "visiting order").
//
// WALK TILES.  The verify kernel stages a stretch of consecutive positions in LDS and walks it query by query; how often its
// insertion chain runs depends on how many pieces -- (query, tile) SEGMENTS -- a query is cut into: every further segment of
// a query arrives with its best documents first and re-admits about K / (segments so far) of them into every lane's list
// (tools/sim_verify_lanes.py --mode tiles: 7.5 of the ~25 admissions per lane and query at 64 positions per tile and 2.9
// segments per query).  So the stretches are not the 64-position tiles of the feature matrix but WALK TILES made by the host
// at upload (wt_start): up to WT = 128 consecutive positions, cut so that a query of up to WT documents lies in ONE of them
// (longer queries are cut every WT documents); a lane handles WT / 64 documents of the tile in phase S.  1.45 segments per
// query at the 30K shape instead of 2.85.
//
// For every document the tables hold the slot it takes inside its walk tile when its segment is sorted
//   * by x_f descending, for every feature f (xslot: static, made once at upload), and
//   * by a trainer's resident sum R descending (rslot: one table per resident slot, redone every few line searches).
// A slot is a position inside the walk tile (segment start + rank inside the segment).  Ties go to the earlier position
// (storage order: gain descending).
// INVARIANT the verify kernel relies on: inside every segment the slots are a PERMUTATION of the segment's positions
// (phase S scatters each document's word to its slot: a table that is not a permutation would drop or duplicate
// documents).  It holds by construction -- xslot ranks with ties broken by position, rslot sorts keys that end in the
// position -- and whenever the tables are rewritten it is on the stream of the launch that reads them next (rslot_kernel is
// queued in front of the verify launch of the same tick, on the same stream; the slots of different streams are disjoint).
// WHICH permutation it is steers admissions only: neither exactness nor parity rests on the choice.  FR_VERIFY_AUDIT=1
// checks the invariant on the device after every rewrite (order_audit_kernel) next to its value audit.
constexpr uint32_t WT = WALK_TILE;      // positions per walk tile, at most (128: device.hpp, where the host cuts them)
constexpr uint32_t WT_DPL = WT / 64;    // documents per lane of a tile

// seg[p] = first slot | (one past the last slot) << 8 of position p's segment, relative to its walk tile's start; 0 for
// positions outside every query.  idx = the position's own offset in the tile, len = documents in the tile.
__device__ __forceinline__ void order_segment(uint32_t s, uint32_t idx, uint32_t len, uint32_t* lo, uint32_t* hi) {
    *lo = s & 0xFFu;
    *hi = s >> 8;
    if (idx >= len || *hi <= *lo) {  // beyond the tile / padding / a document the dataset does not hold: a segment of its own
        *lo = idx;
        *hi = idx + 1u;
    }
}

// grid (walk tiles, ceil(dq / OQ)); 64 threads, WT_DPL documents each; each block ranks OQ feature quads of one walk tile
constexpr int ORDER_OQ = 2;
__global__ __launch_bounds__(WAVE) void xslot_kernel(const float4* __restrict__ xb, const uint16_t* __restrict__ seg, const uint32_t* __restrict__ wt_start,
                                                     uint32_t np, uint32_t dq, uint32_t d, uint8_t* __restrict__ out) {
    __shared__ float4 xs[ORDER_OQ][WT];
    const uint32_t lane = threadIdx.x;
    const uint32_t pb = wt_start[blockIdx.x];
    const uint32_t len = min(wt_start[blockIdx.x + 1] - pb, WT);  // (a run's last tile: what follows it up to the next tile is padding, in no query)
    const uint32_t j0 = blockIdx.y * ORDER_OQ;
    uint32_t lo[WT_DPL], hi[WT_DPL];
    float4 mine[WT_DPL][ORDER_OQ];
#pragma unroll
    for (uint32_t h = 0; h < WT_DPL; h++) {
        const uint32_t idx = lane + 64u * h;
        const uint32_t p = pb + (idx < len ? idx : 0u);
        order_segment(seg[p], idx, len, &lo[h], &hi[h]);
#pragma unroll
        for (int u = 0; u < ORDER_OQ; u++) {
            const uint32_t j4 = j0 + u < dq ? j0 + u : dq - 1;
            const float4 v = xb[((size_t)(p >> 6) * dq + j4) * 64 + (p & 63u)];
            const float ninf = -__builtin_huge_valf();  // (NaN ranks like -inf: the slots stay a permutation)
            mine[h][u] = make_float4(v.x == v.x ? v.x : ninf, v.y == v.y ? v.y : ninf, v.z == v.z ? v.z : ninf, v.w == v.w ? v.w : ninf);
            xs[u][idx] = mine[h][u];
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t h = 0; h < WT_DPL; h++) {
        const uint32_t idx = lane + 64u * h;
        if (idx >= len) continue;
        uint32_t r[ORDER_OQ][4];
#pragma unroll
        for (int u = 0; u < ORDER_OQ; u++)
#pragma unroll
            for (int k = 0; k < 4; k++) r[u][k] = 0;
        for (uint32_t i = lo[h]; i < hi[h]; i++) {
            const bool before = i < idx;
#pragma unroll
            for (int u = 0; u < ORDER_OQ; u++) {
                const float4 o = xs[u][i];
                r[u][0] += (o.x > mine[h][u].x) || (o.x == mine[h][u].x && before);
                r[u][1] += (o.y > mine[h][u].y) || (o.y == mine[h][u].y && before);
                r[u][2] += (o.z > mine[h][u].z) || (o.z == mine[h][u].z && before);
                r[u][3] += (o.w > mine[h][u].w) || (o.w == mine[h][u].w && before);
            }
        }
#pragma unroll
        for (int u = 0; u < ORDER_OQ; u++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t f = (j0 + u) * 4 + k;
                if (j0 + u < dq && f < d) out[(size_t)f * np + pb + idx] = (uint8_t)(lo[h] + r[u][k]);
            }
    }
}

// The tiles' columns, column-major: out[f][p] = x_f of position p.  The RESIDENT verify kernel reads ONE feature per
// line group; in the tiles that float is one in four of a 1 KB row (16 bytes of traffic per document), here it is 4.
// grid (tiles, ceil(dq / ORDER_OQ)), one wave per block.
__global__ __launch_bounds__(WAVE) void xcol_kernel(const float4* __restrict__ xb, uint32_t np, uint32_t dq, uint32_t d, float* __restrict__ out) {
    const uint32_t lane = threadIdx.x, tile = blockIdx.x;
    const size_t p = (size_t)tile * 64u + lane;
    const uint32_t j0 = blockIdx.y * ORDER_OQ;
    float4 v[ORDER_OQ];
#pragma unroll
    for (int u = 0; u < ORDER_OQ; u++) v[u] = xb[((size_t)tile * dq + (j0 + u < dq ? j0 + u : dq - 1)) * 64 + lane];
#pragma unroll
    for (int u = 0; u < ORDER_OQ; u++) {
        const uint32_t f = (j0 + u) * 4;
        if (j0 + u < dq) {
            if (f + 0 < d) out[(size_t)(f + 0) * np + p] = v[u].x;
            if (f + 1 < d) out[(size_t)(f + 1) * np + p] = v[u].y;
            if (f + 2 < d) out[(size_t)(f + 2) * np + p] = v[u].z;
            if (f + 3 < d) out[(size_t)(f + 3) * np + p] = v[u].w;
        }
    }
}

// R ranks of `nlist` resident slots: grid (ceil(walk tiles / 4)); 256 threads = four waves, each wave one walk tile, every
// listed slot in turn.  The wave SORTS the tile: one 32-bit key per document = segment index << 25 | 18 order bits of -R << 7 |
// offset in the tile, two keys per lane (elements lane and lane + 64), put in ascending order over the 128 elements by a
// bitonic network -- lane exchanges (ds_bpermute) for distances below 64, the lane's own two registers for distance 64; the
// document whose key lands in element j then takes slot j (segments are element ranges in segment order, so slot = segment
// start + rank inside the segment).  18 bits of a float's order (sign, exponent, 9 mantissa bits) decide the order (the
// simulator sees no difference from 7 bits up); equal prefixes fall back to the offset (storage order).
// slot_half[k] = resident slot * 2 + the half that holds its current sums.  wlist: the walk tiles to visit (a view: the ones
// that hold its documents; nullptr: all nw of them).
// One compare-exchange stage over the lanes: partner = lane ^ J inside blocks of KK elements.  Which lanes keep the smaller key
// is a compile-time lane mask (a scalar constant: no per-lane arithmetic in the stage); HI = the lane's second element.
template <uint32_t J, uint32_t KK, uint32_t HI>
__device__ __forceinline__ uint32_t order_exchange(uint32_t key, uint32_t lane) {
    constexpr uint64_t keep_min = [] {
        uint64_t m = 0;
        for (uint32_t l = 0; l < 64; l++) {
            const uint32_t e = l + 64u * HI;
            const bool up = (e & KK) == 0u, lower = (e & J) == 0u;
            if (up == lower) m |= 1ull << l;
        }
        return m;
    }();
    const uint32_t other = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane ^ J) << 2), (int)key);
    const uint32_t mn = key < other ? key : other, mx = key < other ? other : key;
    return ((keep_min >> lane) & 1ull) ? mn : mx;
}
template <uint32_t KK, uint32_t HI>
__device__ __forceinline__ uint32_t order_merge(uint32_t key, uint32_t lane) {
    if constexpr (KK >= 64) key = order_exchange<32, KK, HI>(key, lane);
    if constexpr (KK >= 32) key = order_exchange<16, KK, HI>(key, lane);
    if constexpr (KK >= 16) key = order_exchange<8, KK, HI>(key, lane);
    if constexpr (KK >= 8) key = order_exchange<4, KK, HI>(key, lane);
    if constexpr (KK >= 4) key = order_exchange<2, KK, HI>(key, lane);
    return order_exchange<1, KK, HI>(key, lane);
}
static_assert(WT == 128, "the sort below is the 128-element network (two registers per lane)");
constexpr uint32_t RSLOT_BATCH = 4;  // listed slots whose sums a wave loads before it sorts the first of them
// A listed restart's pending update (the candidate its last line search accepted: rs_par / rs_updf of its staged group
// slot_group[k], the verify kernel's own parameters) is applied to the sums on the way in -- the same arithmetic as the
// verify kernel's phase S, so the ranks are those of the sums the launch behind this one walks, not of the sums one accepted
// step ago (which, early in a job, is most of the model).
__global__ __launch_bounds__(256) void rslot_kernel(const double* __restrict__ res, const int32_t* __restrict__ slot_half,
                                                     const int32_t* __restrict__ slot_group, uint32_t nlist, const double* __restrict__ rs_par,
                                                     const uint32_t* __restrict__ rs_updf, const float* __restrict__ xcol,
                                                     const uint16_t* __restrict__ seg, const uint32_t* __restrict__ wt_start,
                                                     const uint32_t* __restrict__ wlist, uint32_t nw, uint32_t np, uint8_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, wi = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (wi >= nw) return;
    const uint32_t ti = wlist ? wlist[wi] : wi;
    const uint32_t pb = wt_start[ti];
    const uint32_t len = min(wt_start[ti + 1] - pb, WT);
    uint32_t p[2], sidx[2];
    {
        uint32_t lo0, hi0, lo1, hi1;
        p[0] = pb + (lane < len ? lane : 0u);
        p[1] = pb + (lane + 64u < len ? lane + 64u : 0u);
        order_segment(seg[p[0]], lane, len, &lo0, &hi0);
        order_segment(seg[p[1]], lane + 64u, len, &lo1, &hi1);
        // segment index inside the tile: how many elements at or below this one start a segment, minus one
        const uint64_t s0 = __ballot(lo0 == lane), s1 = __ballot(lo1 == lane + 64u);
        const uint64_t upto = (lane >= 63u) ? ~0ull : ((2ull << lane) - 1ull);
        sidx[0] = (uint32_t)__popcll(s0 & upto) - 1u;
        sidx[1] = (uint32_t)__popcll(s0) + (uint32_t)__popcll(s1 & upto) - 1u;
    }
    for (uint32_t k0 = 0; k0 < nlist; k0 += RSLOT_BATCH) {
        float r[RSLOT_BATCH][2];
        int32_t sh[RSLOT_BATCH];
#pragma unroll
        for (uint32_t u = 0; u < RSLOT_BATCH; u++) {  // (the batch's loads are in flight together)
            const uint32_t k = k0 + u < nlist ? k0 + u : nlist - 1;
            sh[u] = slot_half[k];
            double R0 = res[(size_t)sh[u] * np + p[0]], R1 = res[(size_t)sh[u] * np + p[1]];
            const double* par = rs_par + (size_t)slot_group[k] * 6;
            if (par[2] != 0.0) {  // (uniform per listed slot)
                const float* xu = xcol + (size_t)rs_updf[slot_group[k]] * np;
                const double x0 = (double)xu[p[0]], x1 = (double)xu[p[1]];
                R0 = __builtin_fma(x0, par[5], __builtin_fma(-x0, par[4], R0 * par[3]));
                R1 = __builtin_fma(x1, par[5], __builtin_fma(-x1, par[4], R1 * par[3]));
            }
            r[u][0] = (float)R0;
            r[u][1] = (float)R1;
        }
#pragma unroll
        for (uint32_t u = 0; u < RSLOT_BATCH; u++) {
            if (k0 + u >= nlist) break;
            uint32_t key[2];
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                // descending R = ascending key: the float's bits in sort order (negative: all bits flipped; else the sign bit set), inverted
                const uint32_t bits = __float_as_uint(r[u][h] == r[u][h] ? r[u][h] : -__builtin_huge_valf());  // (a NaN sum ranks last: its pair is redone anyway)
                const uint32_t mono = bits ^ ((uint32_t)((int32_t)bits >> 31) | 0x80000000u);
                key[h] = (sidx[h] << 25) | ((~mono >> 14) << 7) | (lane + 64u * h);
            }
            key[0] = order_merge<2, 0>(key[0], lane), key[1] = order_merge<2, 1>(key[1], lane);
            key[0] = order_merge<4, 0>(key[0], lane), key[1] = order_merge<4, 1>(key[1], lane);
            key[0] = order_merge<8, 0>(key[0], lane), key[1] = order_merge<8, 1>(key[1], lane);
            key[0] = order_merge<16, 0>(key[0], lane), key[1] = order_merge<16, 1>(key[1], lane);
            key[0] = order_merge<32, 0>(key[0], lane), key[1] = order_merge<32, 1>(key[1], lane);
            key[0] = order_merge<64, 0>(key[0], lane), key[1] = order_merge<64, 1>(key[1], lane);  // (elements 0..63 ascending, 64..127 descending)
            {  // distance 64: the lane's own pair
                const uint32_t mn = key[0] < key[1] ? key[0] : key[1], mx = key[0] < key[1] ? key[1] : key[0];
                key[0] = mn, key[1] = mx;
            }
            key[0] = order_merge<64, 0>(key[0], lane);  // (inside each half every block of 64 is merged upwards: KK = 128 for both halves)
            key[1] = order_merge<64, 0>(key[1], lane);
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t from = key[h] & 127u;
                if (from < len) out[(size_t)(sh[u] >> 1) * np + pb + from] = (uint8_t)(lane + 64u * h);
            }
        }
    }
}

// every table entry = its own offset in its walk tile: storage order (a fresh resident slot before its first ranking)
__global__ void rslot_identity_kernel(uint8_t* __restrict__ out, const uint8_t* __restrict__ wofs, size_t np, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = wofs[i % np];
}

// FR_VERIFY_AUDIT: the invariant at the head of this file, checked on the device -- inside every segment of the listed walk
// tiles the table's slots are a permutation of the segment's positions.  One wave per tile; *bad counts offending documents.
__global__ __launch_bounds__(256) void order_audit_kernel(const uint8_t* __restrict__ table, const uint16_t* __restrict__ seg,
                                                           const uint32_t* __restrict__ wt_start, const uint32_t* __restrict__ wlist, uint32_t nw,
                                                           unsigned long long* bad) {
    __shared__ uint32_t hits[4][WT];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, wi = blockIdx.x * 4u + w;
    const bool on = wi < nw;
    const uint32_t ti = on ? (wlist ? wlist[wi] : wi) : 0u;
    const uint32_t pb = wt_start[ti];
    const uint32_t len = on ? min(wt_start[ti + 1] - pb, WT) : 0u;
    for (uint32_t h = 0; h < WT_DPL; h++) hits[w][lane + 64u * h] = 0u;
    __syncthreads();
    unsigned long long mine = 0;
    for (uint32_t h = 0; h < WT_DPL; h++) {
        const uint32_t idx = lane + 64u * h;
        if (idx >= len) continue;
        const uint16_t s = seg[pb + idx];
        const uint32_t lo = s & 0xFFu, hi = s >> 8;
        if (hi <= lo) continue;  // not a document
        const uint32_t slot = table[pb + idx];
        if (slot < lo || slot >= hi) mine++;
        else atomicAdd(&hits[w][slot], 1u);
    }
    __syncthreads();
    for (uint32_t h = 0; h < WT_DPL; h++) {
        const uint32_t idx = lane + 64u * h;
        if (idx >= len) continue;
        const uint16_t s = seg[pb + idx];
        if ((s >> 8) > (s & 0xFFu) && hits[w][idx] != 1u) mine++;
    }
    if (mine) atomicAdd(bad, mine);
}

// per-column statistics the host's lane-class rule uses: sum, sum of squares, minimum, maximum, and how many documents
// sit at the column's extremes -- two passes (blockIdx.z: 0 = moments and extremes, 1 = counts at the extremes read back)
struct ColStats {
    double sum, sumsq;
    float mn, mx;
    unsigned long long at_min, at_max;
};
__global__ __launch_bounds__(256) void colstats_kernel(const float4* __restrict__ xb, const uint16_t* __restrict__ seg, uint32_t ntiles, uint32_t dq,
                                                       uint32_t d, int pass, ColStats* __restrict__ st) {
    // block = 4 waves, each wave one tile per step; blockIdx.y = feature quad
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, j4 = blockIdx.y;
    double s[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    float mn[4], mx[4];
    unsigned long long cmin[4] = {0, 0, 0, 0}, cmax[4] = {0, 0, 0, 0};
    float emin[4], emax[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        mn[k] = __builtin_huge_valf();
        mx[k] = -__builtin_huge_valf();
        const uint32_t f = j4 * 4 + k;
        emin[k] = (pass == 1 && f < d) ? st[f].mn : 0.0f;
        emax[k] = (pass == 1 && f < d) ? st[f].mx : 0.0f;
    }
    for (uint32_t t = blockIdx.x * 4 + w; t < ntiles; t += gridDim.x * 4) {
        const uint16_t sg = seg[(size_t)t * 64 + lane];
        if ((sg >> 8) <= (sg & 0xFF)) continue;  // not a document of the dataset
        const float4 v = xb[((size_t)t * dq + j4) * 64 + lane];
        const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (pass == 0) {
                s[k] += (double)x[k];
                s2[k] += (double)x[k] * (double)x[k];
                mn[k] = x[k] < mn[k] ? x[k] : mn[k];
                mx[k] = x[k] > mx[k] ? x[k] : mx[k];
            } else {
                cmin[k] += x[k] == emin[k];
                cmax[k] += x[k] == emax[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t f = j4 * 4 + k;
        if (f >= d) continue;
        if (pass == 0) {
            atomicAdd(&st[f].sum, s[k]);
            atomicAdd(&st[f].sumsq, s2[k]);
            // (float min / max through their ordered integer images: non-negative and negative floats need different directions.
            // A zero goes in as +0.0, by value: -0.0 >= 0.0f holds, but its image is INT_MIN -- as a minimum it would beat
            // every negative float already stored, or not, by the order the atomics land in; as a maximum it would lose to
            // every negative one)
            const float lo = mn[k] + 0.0f, hi = mx[k] + 0.0f;
            if (lo >= 0.0f) atomicMin(reinterpret_cast<int*>(&st[f].mn), __float_as_int(lo));
            else atomicMax(reinterpret_cast<unsigned int*>(&st[f].mn), __float_as_uint(lo));
            if (hi >= 0.0f) atomicMax(reinterpret_cast<int*>(&st[f].mx), __float_as_int(hi));
            else atomicMin(reinterpret_cast<unsigned int*>(&st[f].mx), __float_as_uint(hi));
        } else {
            if (cmin[k]) atomicAdd(&st[f].at_min, cmin[k]);
            if (cmax[k]) atomicAdd(&st[f].at_max, cmax[k]);
        }
    }
}
