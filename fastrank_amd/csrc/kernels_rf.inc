// Part of device.hip (single translation unit; see that file's header).  Random-forest TRAINING on the device
// (src/random_forest.rs:211-408): level-synchronous over every open node of a batch of trees.
//
// Per level the host knows the open ("active") nodes a = 0..A-1, each with its tree and size n_a; every tree of the batch
// samples the same NUMBER of features nf (sampling.rs:47), so a (node, feature slot) pair is segment s = a * nf + fi of
// n_a items.  One level is:
//   rf_key_kernel      one item per (tree, feature slot, sampled instance r): 64-bit key = (segment << 32 | the feature
//                      value as order-preserving bits), payload r.  Instances of closed nodes get the segment id A * nf
//                      and sort to the end.  Items are laid out [tree][feature slot][r], r ascending, so after the
//                      STABLE radix sort (rocPRIM) equal values inside a segment stay in ascending r: the tie order the
//                      oracle fixes for the reference's sort_unstable (random_forest.rs:230).
//   rf_rekey_kernel    (levels after the first) the previous level's sorted keys get their children's segment ids and are
//                      stably sorted by those bits alone: same order as a sort from scratch, a third of the radix passes.
//   rf_gather_kernel   gains in sorted order (sg) and the sorted feature values (sv), contiguous per segment.
//   rf_label_kernel    label min / max per node (label_stats, random_forest.rs:218-221).
//   rf_eval_kernel     one wave per segment, lane = split candidate c = 1..k-1: threshold (c/k) * range + min, its position
//                      by binary search (random_forest.rs:236-255), and the importance of the split -- squared error /
//                      Welford variance summed SEQUENTIALLY over the sorted instances, the reference's association
//                      (random_forest.rs:32-51, stats.rs:66-104); Gini / entropy only need the positive counts (the host
//                      finishes them with its own libm log2, like the oracle).
//   (host)             the reference's selection: drop repeated positions, min_leaf_support, best candidate per
//                      feature and best feature per node, last maximum wins.
//   rf_assign_kernel   the chosen segment's items move to the left / right child (node_of[r]).
//   rf_childsum_kernel compute_output of both children: sequential gain sums in the parent's sorted order / count
//                      (random_forest.rs:32-41, 395-398).

struct RFArgs {
    const float* xb;       // feature tiles
    const float* gain;     // [np] by padded position
    uint32_t dq;
    const uint32_t* roff;  // [T+1] start of each tree's sampled instance list
    const uint32_t* pos;   // [total] padded position of instance r of its tree
    const float* gain_r;   // [total] its gain (= gain[pos[.]], rf_gainr_kernel)
    uint32_t* node_of;     // [total] node key the instance currently belongs to
    uint8_t* side_r;       // [total] the side the instance took at its node's last split (1 left, 2 right; rf_assign_kernel)
    const uint32_t* feats; // [T][nf] feature ids of each tree's sample
    uint32_t T, nf, total;
    const uint32_t* slot_of_key;  // [nkeys] node key -> active slot, or IDX_INVALID
    uint32_t A;                   // active nodes this level
    const uint32_t* act_tree;     // [A]
    const uint32_t* act_n;        // [A]
    const uint64_t* act_off;      // [A+1] start of node a's nf segments in the sorted arrays (= sum of n * nf before it)
    uint64_t* keys;               // [total * nf]
    uint32_t* vals;
    const uint64_t* skeys;        // sorted
    const uint32_t* svals;
    float* sg;                    // [items] gains in sorted order
    float* sv;                    // [items] feature values in sorted order (-0.0 = the instance does not hold the feature, see pres)
    const float* sg_o;            // the previous level's sg / sv (the partition's scatter moves an item's gain and value with its key)
    const float* sv_o;
    // file-loaded datasets: bit f of pres[p * pw + f / 32] = the instance at position p HOLDS feature f (nullptr: all do).
    // An absent value is 0.0 in the tiles and sorts as 0.0 (src/random_forest.rs:228), but FeatureStats -- the min / max the
    // thresholds are placed on -- skips it (src/normalizers.rs:24-29).
    const uint32_t* pres;
    uint32_t pw;
    // every label of the dataset is an integer of magnitude <= 2^21: a sum of up to 2^31 of them has only exactly representable
    // partial sums (< 2^53), so it is the same f64 in any order -- the gain sums of a split need no sequential chain
    uint32_t labels_int;
};

__device__ __forceinline__ uint32_t rf_float_key(float x) {
    if (x == 0.0f) x = 0.0f;  // -0.0 and +0.0 compare equal in the reference (NotNan<f64>): one key
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float rf_key_float(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
// first index t in [0, n) with tab[t + 1] > x (tab ascending, tab[0] <= x < tab[n])
template <typename T>
__device__ __forceinline__ uint32_t rf_find_block(const T* tab, uint32_t n, T x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void rf_key_kernel(RFArgs a) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;  // index into the concatenated instance lists
    if (g >= a.total) return;
    const uint32_t t = rf_find_block(a.roff, a.T, g);
    const uint32_t r = g - a.roff[t], nt = a.roff[t + 1] - a.roff[t];
    const uint32_t p = a.pos[g];
    const uint32_t slot = a.slot_of_key[a.node_of[g]];
    const uint64_t base = (uint64_t)a.roff[t] * a.nf;
    for (uint32_t fi = 0; fi < a.nf; fi++) {
        const float x = a.xb[xb_index(p, a.feats[(size_t)t * a.nf + fi], a.dq)];
        const uint64_t seg = slot == IDX_INVALID ? (uint64_t)a.A * a.nf : (uint64_t)slot * a.nf + fi;
        const uint64_t i = base + (uint64_t)fi * nt + r;
        a.keys[i] = (seg << 32) | rf_float_key(x);
        a.vals[i] = r;
    }
}

// Levels after the first: the previous level left every open node's items sorted by (value, r) per feature slot, so a
// STABLE sort by the new segment id alone (the children's slots; closed nodes last) yields the same order as sorting
// from scratch -- this kernel rewrites the segment half of the previous level's sorted keys (old_* = that level's tables).
__global__ __launch_bounds__(256) void rf_rekey_kernel(RFArgs a, uint64_t old_items, uint32_t old_A, uint32_t new_A) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= old_items) return;
    const uint64_t key = a.skeys[i];
    const uint32_t oseg = (uint32_t)(key >> 32);  // the item's segment at the previous level = old slot * nf + feature slot
    const uint32_t na = oseg / a.nf, fi = oseg % a.nf;
    const uint32_t r = a.svals[i];
    const uint32_t slot = a.slot_of_key[a.node_of[a.roff[a.act_tree[na]] + r]];
    const uint64_t seg = slot == IDX_INVALID ? (uint64_t)new_A * a.nf : (uint64_t)slot * a.nf + fi;
    a.keys[i] = (seg << 32) | (key & 0xFFFFFFFFull);
    a.vals[i] = r;
}

// the feature value of a sorted item as rf_eval_kernel wants it: the key's value bits (a held zero comes back as +0.0:
// rf_float_key folds -0.0 onto it), or -0.0 -- the marker for "the instance does not hold this feature" -- on file-loaded datasets
__device__ __forceinline__ float rf_sorted_value(const RFArgs& a, uint32_t t, uint32_t fi, uint32_t g, uint32_t keybits) {
    float val = rf_key_float(keybits);
    if (a.pres != nullptr) {
        const uint32_t p = a.pos[g];
        const uint32_t f = a.feats[(size_t)t * a.nf + fi];
        if (((a.pres[(size_t)p * a.pw + (f >> 5)] >> (f & 31u)) & 1u) == 0u) val = -0.0f;
    }
    return val;
}

// once per batch: the gain of every sampled instance, by its index in the batch's instance lists, and its first node (the
// root of its tree: key t)
__global__ __launch_bounds__(256) void rf_gainr_kernel(const float* gain, const uint32_t* pos, const uint32_t* roff, uint32_t T, float* gain_r,
                                                       uint32_t* node_of, uint32_t total) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    gain_r[g] = gain[pos[g]];
    node_of[g] = rf_find_block(roff, T, g);
}

__global__ __launch_bounds__(256) void rf_gather_kernel(RFArgs a, uint64_t items) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= items) return;
    const uint64_t key = a.skeys[i];
    const uint32_t na = (uint32_t)(key >> 32) / a.nf;  // the sorted key carries its segment = slot * nf + feature slot
    const uint32_t t = a.act_tree[na];
    const uint32_t g = a.roff[t] + a.svals[i];
    a.sg[i] = a.gain_r[g];
    a.sv[i] = rf_sorted_value(a, t, (uint32_t)(key >> 32) % a.nf, g, (uint32_t)key);
}

// one workgroup per active node: min / max label over the node's instances (feature slot 0's segment).  Sixteen waves: the
// first levels have a handful of nodes of a million instances each (one wave per node took 7.6 ms per level there, PMC r03)
constexpr int RF_LABEL_THREADS = 1024;
__global__ __launch_bounds__(RF_LABEL_THREADS) void rf_label_kernel(RFArgs a, float* out /*[A][2]*/) {
    __shared__ float slo[RF_LABEL_THREADS / 64], shi[RF_LABEL_THREADS / 64];
    const uint32_t na = blockIdx.x;
    const float* g = a.sg + a.act_off[na];
    const uint32_t n = a.act_n[na];
    float lo = __builtin_huge_valf(), hi = -__builtin_huge_valf();
    for (uint32_t i = threadIdx.x; i < n; i += RF_LABEL_THREADS) {
        lo = fminf(lo, g[i]);
        hi = fmaxf(hi, g[i]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
    }
    if ((threadIdx.x & 63u) == 0) slo[threadIdx.x >> 6] = lo, shi[threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RF_LABEL_THREADS / 64; w++) lo = fminf(lo, slo[w]), hi = fmaxf(hi, shi[w]);
        out[na * 2] = lo;
        out[na * 2 + 1] = hi;
    }
}

struct RfCandDev {
    double position;    // the threshold (random_forest.rs:238)
    double importance;  // methods 0 / 3; NaN marks "the reference would have panicked" (variance of < 2 labels)
    uint32_t ids_i;     // instances strictly below the threshold
    uint32_t flags;     // 1: evaluated (a new position with both sides >= min_leaf_support); the reference panics on this
                        // (node, feature) if the node's labels differ -- 2: a NaN among its values, 4: a NaN position (rf_eval_kernel)
    uint32_t pos_l, pos_r;  // instances with gain > 0 on each side (methods 1 / 2)
    double sum_l, sum_r;    // method 0: the sequential gain sums of both sides in this segment's order -- what compute_output of
                            // the children divides by their sizes (random_forest.rs:32-41, 395-398) if this candidate is chosen
};

__device__ __forceinline__ uint32_t rf_lower_bound(const float* v, uint32_t n, double position) {
    uint32_t lo = 0, hi = n;  // first index whose value is not < position
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((double)v[mid] < position) lo = mid + 1; else hi = mid;
    }
    return lo;
}

constexpr uint32_t RF_CHUNK = 512;  // gains staged per trip (one coalesced load by the wave, then broadcast reads)

// A segment's gains, streamed through LDS one chunk at a time with the NEXT chunk's loads already in flight (registers)
// while the current one is summed: the sequential chains never wait for global memory.  Chunks are zero-padded.
struct RfStream {
    const float* g;
    uint32_t n, lane;
    float pre[RF_CHUNK / 64];
    __device__ __forceinline__ void fetch(uint32_t base) {
#pragma unroll
        for (uint32_t u = 0; u < RF_CHUNK / 64; u++) {
            const uint32_t j = base + u * 64 + lane;
            pre[u] = j < n ? g[j] : 0.0f;
        }
    }
    __device__ __forceinline__ void begin(const float* g_, uint32_t n_, uint32_t lane_) {
        g = g_;
        n = n_;
        lane = lane_;
        fetch(0);
    }
    // buf <- the chunk at `base` (fetched before); starts fetching the one after it
    __device__ __forceinline__ void stage(double* buf, uint32_t base) {
        __syncthreads();
#pragma unroll
        for (uint32_t u = 0; u < RF_CHUNK / 64; u++) buf[u * 64 + lane] = (double)pre[u];
        __syncthreads();
        if (base + RF_CHUNK < n) fetch(base + RF_CHUNK);
    }
};


// acc + buf[0] + buf[1] + .. + buf[cnt-1], added one after the other (the reference's association), for cnt a multiple of 16.
// The time of a level is the time of its LONGEST chain -- the thresholds sit at fractions of the value RANGE, so a skewed column
// leaves one child almost as long as its parent at every depth -- and a chain advances one dependent v_add_f64 per element: the
// LDS reads must never be waited for.  Sixteen values are kept in registers, eight being added while the next eight are read.
// SQ: the terms are (mm - x)^2 (formed off the chain).  Reads up to 16 doubles past cnt (the chunk buffer is that much longer).
template <bool SQ>
__device__ __forceinline__ double rf_chain16(const double* __restrict__ buf, uint32_t cnt, double acc, double mm) {
    double xa[8], xb[8];
    auto ld8 = [&](double (&x)[8], const double* p) {
        const double2 t0 = reinterpret_cast<const double2*>(p)[0], t1 = reinterpret_cast<const double2*>(p)[1];
        const double2 t2 = reinterpret_cast<const double2*>(p)[2], t3 = reinterpret_cast<const double2*>(p)[3];
        x[0] = t0.x, x[1] = t0.y, x[2] = t1.x, x[3] = t1.y, x[4] = t2.x, x[5] = t2.y, x[6] = t3.x, x[7] = t3.y;
        if (SQ) {
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const double d = mm - x[u];
                x[u] = d * d;
            }
        }
    };
    ld8(xa, buf);
    for (uint32_t e = 0; e < cnt; e += 16) {
        ld8(xb, buf + e + 8);
#pragma unroll
        for (int u = 0; u < 8; u++) acc += xa[u];
        ld8(xa, buf + e + 16);
#pragma unroll
        for (int u = 0; u < 8; u++) acc += xb[u];
    }
    return acc;
}

// inclusive prefix sum over the 64 lanes of a wave, DPP only (no trip through the LDS crossbar): within rows of 16, then
// across the rows
__device__ __forceinline__ int32_t rf_wave_scan(int32_t x) {
#define RF_DPP(src, ctrl, rmask, bmask) __builtin_amdgcn_update_dpp(0, (src), (ctrl), (rmask), (bmask), false)
    int32_t s = x + RF_DPP(x, 0x111, 0xF, 0xF);   // row_shr:1
    s += RF_DPP(x, 0x112, 0xF, 0xF);               // row_shr:2
    s += RF_DPP(x, 0x113, 0xF, 0xF);               // row_shr:3
    s += RF_DPP(s, 0x114, 0xF, 0xE);               // row_shr:4, lanes 4..15 of a row
    s += RF_DPP(s, 0x118, 0xF, 0xC);               // row_shr:8, lanes 8..15
    s += RF_DPP(s, 0x142, 0xA, 0xF);               // row_bcast:15 into rows 1 and 3
    s += RF_DPP(s, 0x143, 0xC, 0xF);               // row_bcast:31 into rows 2 and 3
#undef RF_DPP
    return s;
}

// One WAVE per segment (node, feature slot); lane = split candidate c = 1..k-1 (blocks of 64 candidates when k > 65).
// The segment's gains are streamed through LDS chunk by chunk -- loaded once by the whole wave, then read by every
// lane at the same address (a broadcast) -- and every lane runs its own sequential sums over them: the reference's
// association for each candidate, at the cost of one pass for the whole wave.  A value that belongs to the other side
// of a lane's split is added as +0.0, which never changes a sum that starts at +0.0 (it cannot be -0.0).
__global__ __launch_bounds__(64) void rf_eval_kernel(RFArgs a, uint32_t k, int method, uint32_t min_leaf, RfCandDev* out) {
    __shared__ double buf[RF_CHUNK + 16];  // (+16: rf_chain16 reads ahead; kept zero)
    if (threadIdx.x < 16) buf[RF_CHUNK + threadIdx.x] = 0.0;
    const uint32_t lane = threadIdx.x;
    const uint32_t km1 = k - 1;
    const uint64_t s = blockIdx.x;
    const uint32_t na = (uint32_t)(s / a.nf), fi = (uint32_t)(s % a.nf);
    const uint32_t n = a.act_n[na];
    const uint64_t off = a.act_off[na] + (uint64_t)fi * n;
    const float* v = a.sv + off;
    const float* g = a.sg + off;
    // FeatureStats of this (node, feature): min / max over the values the node's instances hold and how many there are.
    // Everything held (the usual case): the ends of the sorted segment.
    // Non-finite values: StreamingStats::push (stats.rs:46-47, 74-79) starts at min = f64::MAX, max = f64::MIN and compares with
    // > and <, so a NaN is counted but becomes neither, a segment of nothing but +inf keeps min = f64::MAX and one of nothing but
    // -inf keeps max = f64::MIN.  A NaN among the segment's values (Scored::new, random_forest.rs:228) or a NaN position
    // (NotNan::new(..).unwrap(), :238 -- a minimum of -inf) is a panic there: flags 2 and 4 of every candidate of the segment, for the
    // host to raise once it knows that the node's labels differ.  rf_float_key sorts a NaN of the sign bit's side below -inf and the
    // others above +inf, so the ends of the sorted segment show one of either kind.
    double fmin = 0.0, fmax = 0.0;
    uint32_t held = n;
    bool has_nan = false;
    if (a.pres == nullptr) {
        if (n > 0) {
            const float v0 = v[0], v1 = v[n - 1];
            has_nan = v0 != v0 || v1 != v1;
            fmin = v0 == __builtin_huge_valf() ? 1.7976931348623157e308 : (double)v0;
            fmax = v1 == -__builtin_huge_valf() ? -1.7976931348623157e308 : (double)v1;
        }
    } else {
        // (an absent value reads 0.0 in the reference's sort, never NaN: only held values are looked at)
        float lo = 3.4028234663852886e38f, hi = -3.4028234663852886e38f;
        uint32_t cnt = 0, nans = 0;
        for (uint32_t i = lane; i < n; i += 64) {
            const float x = v[i];
            const bool absent = __float_as_uint(x) == 0x80000000u;
            if (!absent) {
                lo = fminf(lo, x);
                hi = fmaxf(hi, x);
                cnt++;
                nans += x != x ? 1u : 0u;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o));
            hi = fmaxf(hi, __shfl_xor(hi, o));
            cnt += __shfl_xor(cnt, o);
            nans += __shfl_xor(nans, o);
        }
        held = cnt;
        has_nan = nans != 0;
        fmin = (double)lo, fmax = (double)hi;
    }
    for (uint32_t cb = 0; cb < km1; cb += 64) {
        const uint32_t c = cb + lane + 1;
        const bool have = c <= km1;
        RfCandDev r;
        r.position = 0.0;
        r.importance = 0.0;
        r.ids_i = 0;
        r.flags = 0;
        r.pos_l = r.pos_r = 0;
        r.sum_l = r.sum_r = 0.0;
        bool valid = false;
        uint32_t nl = 0;
        if (have && n > 1 && held > 1) {  // FeatureStats needs > 1 element (stats.rs:98-103)
            const double range = fmax - fmin;
            const double frac = (double)c / (double)k;
            const double position = frac * range + fmin;
            const uint32_t ids_i = rf_lower_bound(v, n, position);
            r.position = position;
            r.ids_i = ids_i;
            r.flags = (has_nan ? 2u : 0u) | (position != position ? 4u : 0u);
            bool fresh = true;  // random_forest.rs:249-253: a position equal to the previously pushed one is skipped
            if (c > 1) {
                const double fprev = (double)(c - 1) / (double)k;
                fresh = rf_lower_bound(v, n, fprev * range + fmin) != ids_i;
            }
            nl = ids_i;
            valid = fresh && nl >= min_leaf && (n - nl) >= min_leaf;
        }
        if (__any(valid)) {  // (uniform: the loops below contain block barriers)
            RfStream st;
            const uint32_t nr = n - nl;
            if (valid) r.flags |= 1;
            if (method == 0) {  // SquaredError: -(sum_l (mean_l - g)^2 + sum_r (mean_r - g)^2), random_forest.rs:42-51,97-99
                // A chunk lies entirely on one side of a lane's split except for the one chunk that contains it: when no
                // lane's split falls into the chunk (the common case) every lane adds the whole chunk to ONE of its two
                // chains -- one dependent v_add_f64 per element, LDS reads four elements ahead.
                double sl = 0.0, sr = 0.0;
                if (a.labels_int) {
                    // integer labels (RFArgs::labels_int): the two sums in integer arithmetic, 64 instances per trip -- a wave
                    // scan of the trip, lane c takes the prefix below its own split.  Same f64 as the sequential sums, and
                    // half of this method's chain is gone.
                    int64_t il = 0, ir = 0;
                    RfStream st1;  // (the next eight trips' loads are in flight while these eight are scanned)
                    st1.begin(g, n, lane);
                    for (uint32_t base = 0; base < n; base += RF_CHUNK) {
                        float cur[RF_CHUNK / 64];
#pragma unroll
                        for (uint32_t u = 0; u < RF_CHUNK / 64; u++) cur[u] = st1.pre[u];
                        if (base + RF_CHUNK < n) st1.fetch(base + RF_CHUNK);
#pragma unroll
                        for (uint32_t u = 0; u < RF_CHUNK / 64; u++) {
                            const uint32_t b0 = base + u * 64;
                            const int32_t sc = rf_wave_scan((int32_t)cur[u]);  // (zero beyond n)
                            const int32_t tot = __builtin_amdgcn_readlane(sc, 63);
                            const uint32_t below = nl > b0 ? (nl - b0 < 64u ? nl - b0 : 64u) : 0u;
                            const int32_t pre = __builtin_amdgcn_ds_bpermute((int)((below ? below - 1u : 0u) << 2), sc);
                            const int32_t left = below ? pre : 0;
                            il += left;
                            ir += tot - left;
                        }
                    }
                    sl = (double)il, sr = (double)ir;
                } else {
                st.begin(g, n, lane);
                for (uint32_t base = 0; base < n; base += RF_CHUNK) {
                    const uint32_t cnt = n - base < RF_CHUNK ? n - base : RF_CHUNK;
                    st.stage(buf, base);
                    const bool all_left = base + cnt <= nl, all_right = base >= nl;
                    if (__all(all_left || all_right)) {
                        // (the chunk is zero-padded: adding +0.0 is the identity, so the count is rounded up to 16)
                        const double acc = rf_chain16<false>(buf, (cnt + 15u) & ~15u, all_left ? sl : sr, 0.0);
                        sl = all_left ? acc : sl;
                        sr = all_left ? sr : acc;
                    } else {
                        for (uint32_t e = 0; e < cnt; e++) {
                            const double x = buf[e];
                            const bool left = base + e < nl;
                            sl += left ? x : 0.0;
                            sr += left ? 0.0 : x;
                        }
                    }
                }
                }
                r.sum_l = sl, r.sum_r = sr;
                const double ml = nl ? sl / (double)nl : 0.0, mr = nr ? sr / (double)nr : 0.0;
                double el = 0.0, er = 0.0;
                st.begin(g, n, lane);
                for (uint32_t base = 0; base < n; base += RF_CHUNK) {
                    const uint32_t cnt = n - base < RF_CHUNK ? n - base : RF_CHUNK;
                    st.stage(buf, base);
                    const bool all_left = base + cnt <= nl, all_right = base >= nl;
                    if (__all(all_left || all_right)) {
                        const double mm = all_left ? ml : mr;
                        uint32_t e = cnt & ~15u;  // (the padding is not an instance here: its term would be mm^2)
                        double acc = rf_chain16<true>(buf, e, all_left ? el : er, mm);
                        for (; e < cnt; e++) {
                            const double d = mm - buf[e];
                            acc += d * d;
                        }
                        el = all_left ? acc : el;
                        er = all_left ? er : acc;
                    } else {
                        for (uint32_t e = 0; e < cnt; e++) {
                            const double x = buf[e];
                            const bool left = base + e < nl;
                            const double d = (left ? ml : mr) - x;
                            const double sq = d * d;
                            el += left ? sq : 0.0;
                            er += left ? 0.0 : sq;
                        }
                    }
                }
                r.importance = -(el + er);
            } else if (method == 3) {  // TrueVarianceReduction: Welford per side (stats.rs:66-104), random_forest.rs:116-122
                double mean[2] = {0.0, 0.0}, ss[2] = {0.0, 0.0};
                st.begin(g, n, lane);
                for (uint32_t base = 0; base < n; base += RF_CHUNK) {
                    const uint32_t cnt = n - base < RF_CHUNK ? n - base : RF_CHUNK;
                    st.stage(buf, base);
                    if (valid) {
                        for (uint32_t e = 0; e < cnt; e++) {
                            const double x = buf[e];
                            const uint32_t i = base + e;
                            const int side = i < nl ? 0 : 1;
                            const uint32_t first = side ? nl : 0;
                            if (i == first) {
                                mean[side] = x;
                            } else {
                                const double old_mean = mean[side];
                                mean[side] = old_mean + (x - old_mean) / (double)(i - first + 1);
                                ss[side] = ss[side] + (x - old_mean) * (x - mean[side]);
                            }
                        }
                    }
                }
                const bool ok = nl > 1 && nr > 1;  // label_stats(..).unwrap(): finish() is None below two elements
                r.importance = ok ? -((ss[0] / (double)(nl - 1)) * (double)nl + (ss[1] / (double)(nr - 1)) * (double)nr) : __builtin_nan("");
            } else {  // Gini / entropy: the positive counts (the host finishes them with its libm)
                // Counting is associative: no chain.  The wave reads 64 gains at a time; their "positive" bits are one wave mask,
                // and lane c takes the bits below its own split position -- a handful of instructions per 64 instances,
                // however many candidates there are.
                uint32_t pl = 0, ptot = 0;
                for (uint32_t base = 0; base < n; base += 64) {
                    const uint32_t j = base + lane;
                    const uint64_t pos = __ballot(j < n && g[j] > 0.0f);
                    const uint32_t below = nl > base ? (nl - base < 64u ? nl - base : 64u) : 0u;  // instances of this trip left of the lane's split
                    const uint64_t mine = below >= 64u ? pos : (pos & ((1ull << below) - 1ull));
                    pl += (uint32_t)__builtin_popcountll(mine);
                    ptot += (uint32_t)__builtin_popcountll(pos);
                }
                r.pos_l = pl;
                r.pos_r = ptot - pl;
            }
            if (!valid) {  // (a lane that only walked along with its block: nothing of its walk is part of the record)
                r.importance = 0.0;
                r.pos_l = r.pos_r = 0;
                r.sum_l = r.sum_r = 0.0;
            }
        }
        if (have) out[s * km1 + (c - 1)] = r;
    }
}


struct RfSplitDev {
    int32_t fslot;  // chosen feature slot, or -1: the node becomes a leaf
    uint32_t pos, left, right;
};

__global__ __launch_bounds__(256) void rf_assign_kernel(RFArgs a, const RfSplitDev* sp, uint64_t node_items /*sum of n_a*/,
                                                       const uint64_t* act_first /*[A+1] prefix of n_a*/) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= node_items) return;
    const uint32_t na = rf_find_block(act_first, a.A, i);
    const RfSplitDev s = sp[na];
    if (s.fslot < 0) return;
    const uint32_t j = (uint32_t)(i - act_first[na]), n = a.act_n[na];
    const uint32_t r = a.svals[a.act_off[na] + (uint64_t)s.fslot * n + j];
    const uint32_t g = a.roff[a.act_tree[na]] + r;
    a.node_of[g] = j < s.pos ? s.left : s.right;
    a.side_r[g] = j < s.pos ? 1 : 2;  // (one byte per instance: the partition of the next level gathers this, not the 4-byte key)
}

// ---- levels after the first: the children's segments by STABLE PARTITION of the parent's -------------------------------------
// A node's items are sorted by (value, r) in each of its nf segments; its children's segments are those items, in that order, split
// by the side the instance went to (rf_assign_kernel).  rf_rekey_kernel + a stable radix sort by segment id does exactly that with
// three passes over 12-byte items and a library sort; these three kernels do it with one and a half: count per tile of RF_PT
// items (the side of every item is kept as one byte), an exclusive scan of the tiles of each segment, and a scatter to
//     new offset of the child + feature slot * child size + items of that child earlier in the segment.
// Same arrays as the sort would leave (tests/test_gpu_rf_levels.py compares svals / sv / sg of every level with the sort's, under
// FR_RF_PARTITION=0, and with tests/rf_level_model.py's definition).
constexpr uint32_t RF_PT = 2048;  // items per tile: 256 threads x 8
struct RFPart {
    const uint32_t* o_tree;         // the PREVIOUS level's tables
    const uint32_t* o_n;
    const uint64_t* o_off;
    const uint64_t* o_tile_first;   // [o_A + 1] first tile of node a's nf segments (each has ceil(n / RF_PT) tiles)
    uint32_t o_A;
    const RfSplitDev* sp;           // the previous level's decisions
    uint32_t* tile_cnt;             // [tiles][2] left / right items of the tile, then their exclusive prefix within the segment
    uint8_t* side;                  // [items of the previous level] 0: dropped (closed child), 1: left, 2: right
};
struct RFTile {
    uint32_t na, fi, tl, n, cnt;
    uint64_t first;  // index of the tile's first item in the previous level's sorted arrays
};
__device__ __forceinline__ RFTile rf_tile_of(const RFArgs& a, const RFPart& p, uint32_t tile) {
    RFTile t;
    t.na = rf_find_block(p.o_tile_first, p.o_A, (uint64_t)tile);
    t.n = p.o_n[t.na];
    const uint32_t tps = (t.n + RF_PT - 1) / RF_PT, local = tile - (uint32_t)p.o_tile_first[t.na];
    t.fi = local / tps;
    t.tl = local % tps;
    const uint32_t i0 = t.tl * RF_PT;
    t.cnt = t.n - i0 < RF_PT ? t.n - i0 : RF_PT;
    t.first = p.o_off[t.na] + (uint64_t)t.fi * t.n + i0;
    return t;
}

__global__ __launch_bounds__(256) void rf_part_count_kernel(RFArgs a, RFPart p) {
    __shared__ uint32_t red[2][4];
    const uint32_t tile = blockIdx.x, tid = threadIdx.x;
    const RFTile t = rf_tile_of(a, p, tile);
    const RfSplitDev s = p.sp[t.na];
    uint32_t cl = 0, cr = 0;
    if (s.fslot >= 0) {
        const bool okl = a.slot_of_key[s.left] != IDX_INVALID, okr = a.slot_of_key[s.right] != IDX_INVALID;
        if (okl || okr) {
            const uint32_t rbase = a.roff[p.o_tree[t.na]];
#pragma unroll
            for (uint32_t j = 0; j < RF_PT / 256; j++) {
                const uint32_t idx = j * 256 + tid;
                if (idx < t.cnt) {
                    const uint32_t took = a.side_r[rbase + a.svals[t.first + idx]];
                    const uint32_t sd = (took == 1u && okl) ? 1u : ((took == 2u && okr) ? 2u : 0u);
                    p.side[t.first + idx] = (uint8_t)sd;
                    cl += sd == 1u, cr += sd == 2u;
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) cl += __shfl_xor(cl, o), cr += __shfl_xor(cr, o);
    if ((tid & 63u) == 0) red[0][tid >> 6] = cl, red[1][tid >> 6] = cr;
    __syncthreads();
    if (tid == 0) {
        p.tile_cnt[2 * (size_t)tile] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        p.tile_cnt[2 * (size_t)tile + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

// one wave per segment of the previous level: the tiles' counts become exclusive prefixes
__global__ __launch_bounds__(64) void rf_part_scan_kernel(RFArgs a, RFPart p) {
    const uint32_t seg = blockIdx.x, lane = threadIdx.x;
    const uint32_t na = seg / a.nf, fi = seg % a.nf;
    const uint32_t n = p.o_n[na], tps = (n + RF_PT - 1) / RF_PT;
    uint32_t* c = p.tile_cnt + 2 * ((size_t)p.o_tile_first[na] + (size_t)fi * tps);
    int32_t carry_l = 0, carry_r = 0;
    for (uint32_t t0 = 0; t0 < tps; t0 += 64) {
        const uint32_t t = t0 + lane;
        const int32_t xl = t < tps ? (int32_t)c[2 * t] : 0, xr = t < tps ? (int32_t)c[2 * t + 1] : 0;
        const int32_t sl = rf_wave_scan(xl), sr = rf_wave_scan(xr);
        if (t < tps) c[2 * t] = (uint32_t)(carry_l + sl - xl), c[2 * t + 1] = (uint32_t)(carry_r + sr - xr);
        carry_l += __builtin_amdgcn_readlane(sl, 63);
        carry_r += __builtin_amdgcn_readlane(sr, 63);
    }
}

__global__ __launch_bounds__(256) void rf_part_scatter_kernel(RFArgs a, RFPart p) {
    __shared__ uint32_t cnt[RF_PT / 256][4][2], base[RF_PT / 256][4][2];
    const uint32_t tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const RFTile t = rf_tile_of(a, p, tile);
    const RfSplitDev s = p.sp[t.na];
    if (s.fslot < 0) return;
    const uint32_t slot_l = a.slot_of_key[s.left], slot_r = a.slot_of_key[s.right];
    if (slot_l == IDX_INVALID && slot_r == IDX_INVALID) return;
    uint32_t sd[RF_PT / 256], intra[RF_PT / 256];
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (uint32_t j = 0; j < RF_PT / 256; j++) {
        const uint32_t idx = j * 256 + tid;
        sd[j] = idx < t.cnt ? p.side[t.first + idx] : 0u;
        const uint64_t ml = __ballot(sd[j] == 1u), mr = __ballot(sd[j] == 2u);
        intra[j] = (uint32_t)__builtin_popcountll((sd[j] == 1u ? ml : mr) & below);
        if (lane == 0) cnt[j][wave][0] = (uint32_t)__builtin_popcountll(ml), cnt[j][wave][1] = (uint32_t)__builtin_popcountll(mr);
    }
    __syncthreads();
    if (tid < 2) {  // items of this side before each (row, wave) of the tile, in item order
        uint32_t run = p.tile_cnt[2 * (size_t)tile + tid];
        for (uint32_t j = 0; j < RF_PT / 256; j++)
            for (uint32_t w = 0; w < 4; w++) base[j][w][tid] = run, run += cnt[j][w][tid];
    }
    __syncthreads();
    const uint64_t dst_l = slot_l != IDX_INVALID ? a.act_off[slot_l] + (uint64_t)t.fi * a.act_n[slot_l] : 0;
    const uint64_t dst_r = slot_r != IDX_INVALID ? a.act_off[slot_r] + (uint64_t)t.fi * a.act_n[slot_r] : 0;
    const uint64_t seg_l = ((uint64_t)slot_l * a.nf + t.fi) << 32, seg_r = ((uint64_t)slot_r * a.nf + t.fi) << 32;
#pragma unroll
    for (uint32_t j = 0; j < RF_PT / 256; j++) {
        if (sd[j] == 0u) continue;
        const uint64_t i = t.first + j * 256 + tid;
        const bool left = sd[j] == 1u;
        const uint64_t d = (left ? dst_l : dst_r) + base[j][wave][left ? 0 : 1] + intra[j];
        const uint32_t keybits = (uint32_t)a.skeys[i], r = a.svals[i];
        a.keys[d] = (left ? seg_l : seg_r) | keybits;
        a.vals[d] = r;
        // (what rf_gather_kernel would write for the new level -- the item's gain and value travel with it: no second pass over
        // the sorted items, no gather by instance)
        a.sg[d] = a.sg_o[i];
        a.sv[d] = a.sv_o[i];
    }
}

// one wave per active node: gain_sum / len of both children over the child's instances in the parent's sorted order
// (chunks staged in LDS by the whole wave; the sum itself is one sequential chain, computed by every lane alike)
__global__ __launch_bounds__(64) void rf_childsum_kernel(RFArgs a, const RfSplitDev* sp, double* out /*[A][2]*/) {
    __shared__ double buf[RF_CHUNK + 16];
    if (threadIdx.x < 16) buf[RF_CHUNK + threadIdx.x] = 0.0;
    const uint32_t na = blockIdx.x, lane = threadIdx.x;
    const RfSplitDev s = sp[na];
    if (s.fslot < 0) {
        if (lane < 2) out[na * 2 + lane] = 0.0;
        return;
    }
    const uint32_t n = a.act_n[na];
    const float* g = a.sg + a.act_off[na] + (uint64_t)s.fslot * n;
    double sum[2] = {0.0, 0.0};
    RfStream st;
    st.begin(g, n, lane);
    for (uint32_t base = 0; base < n; base += RF_CHUNK) {
        const uint32_t cnt = n - base < RF_CHUNK ? n - base : RF_CHUNK;
        st.stage(buf, base);
        if (base + cnt <= s.pos || base >= s.pos) {  // the whole chunk belongs to one child (zero padding: +0.0 is the identity)
            const double acc = rf_chain16<false>(buf, (cnt + 15u) & ~15u, base >= s.pos ? sum[1] : sum[0], 0.0);
            if (base >= s.pos) sum[1] = acc; else sum[0] = acc;
        } else {
            for (uint32_t e = 0; e < cnt; e++) {
                const double x = buf[e];
                const bool left = base + e < s.pos;
                sum[0] += left ? x : 0.0;
                sum[1] += left ? 0.0 : x;
            }
        }
    }
    if (lane == 0) {
        out[na * 2] = s.pos ? sum[0] / (double)s.pos : 0.0;
        out[na * 2 + 1] = n > s.pos ? sum[1] / (double)(n - s.pos) : 0.0;
    }
}

// one wave per tree: compute_output of the whole sample in list order (only asked for when a root does not split)
__global__ __launch_bounds__(64) void rf_rootsum_kernel(RFArgs a, double* out /*[T]*/) {
    __shared__ double buf[RF_CHUNK];
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    const uint32_t b = a.roff[t], n = a.roff[t + 1] - b;
    double sum = 0.0;
    for (uint32_t base = 0; base < n; base += RF_CHUNK) {
        const uint32_t cnt = n - base < RF_CHUNK ? n - base : RF_CHUNK;
        __syncthreads();
        for (uint32_t j = lane; j < cnt; j += 64) buf[j] = (double)a.gain[a.pos[b + base + j]];
        __syncthreads();
        for (uint32_t e = 0; e < cnt; e++) sum += buf[e];
    }
    if (lane == 0) out[t] = n ? sum / (double)n : 0.0;
}
