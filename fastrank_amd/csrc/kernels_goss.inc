// Part of device.hip (single translation unit; see that file's header).  LambdaMART's gradient-based one-side sampling
// (DESIGN.md section 11, "GOSS"): a tree of the histogram grower is fitted to the n_top documents of its instance list L with
// the largest |lambda| and to a Bernoulli sample of the others, whose gradients are amplified.
//
//   key_i = the 64 bits of fabs(lambda_i): non-negative doubles order like their bit patterns, and the sign bit is 0
//   goss_hist_kernel / goss_pick_kernel, GOSS_PASSES times
//                         MSB-first radix select of tau = the n_top-th largest key.  Pass p looks at digit p of the keys that
//                         agree with the digits chosen so far: the workgroups count them in LDS (32-bit LDS atomics, one
//                         global atomicAdd per touched bin), then ONE WAVE walks the bins from the largest digit down, picks
//                         the digit that holds the wanted rank and leaves (chosen prefix, remaining rank) in device memory
//                         for the next pass.  No host synchronisation in the chain.  The first pass gathers the keys from
//                         lambda into a dense array the later passes stream.  After the last pass the prefix is tau and the
//                         remaining rank is the number of entries with key == tau that belong to the top set.
//   goss_tie_kernel / (rocPRIM exclusive scan)
//                         flag = key == tau by full-list index; its prefix sums are every tied entry's rank among the ties in
//                         list order
//   goss_flag_kernel / (rocPRIM exclusive scan) / hist_rootlist_kernel
//                         top = key > tau, or key == tau and tie rank < remaining rank; every other entry is kept iff
//                         u < p, u = (mix(K_t + 0x9E3779B97F4A7C15 (id + 1)) >> 11) 2^-53 (xe_gamma's stream under the tree's
//                         GOSS key, id = the document's original instance id); the kept entries' ascending list is the tree's root list
//   goss_absmax_kernel / goss_quant_kernel
//                         hist_absmax_kernel / hist_quant_kernel over that list with the kept others' lambda and w multiplied
//                         by amp first (one rounded product each: -ffp-contract=off)
//
// Digit width: 11 bits.  The sign bit of a key is 0, so 63 bits are left: five digits of 11 bits and a last one of 9 make
// GOSS_PASSES = 6 passes where 8-bit digits need 8, every pass being one read of the keys plus two launches; 2048 u32 bins
// are 8 KiB of LDS (a 2^16-bin histogram would not fit) and 32 bins per lane of the one picking wave.

constexpr uint32_t GOSS_BITS = 11;
constexpr uint32_t GOSS_BINS = 1u << GOSS_BITS;
constexpr uint32_t GOSS_PASSES = 6;
constexpr uint32_t GOSS_SHARE = 4096;  // entries of the list per workgroup of goss_hist_kernel

struct GossStateDev {
    unsigned long long prefix;  // the digits chosen so far, right-aligned; after the last pass: tau
    uint32_t rank;              // the wanted rank (1 = the largest) among the keys that carry the prefix
    uint32_t pad;
};

// digit p of a key: bits [goss_shift(p), goss_shift(p) + goss_width(p))
__host__ __device__ constexpr uint32_t goss_shift(uint32_t p) { return p + 1 < GOSS_PASSES ? 64u - GOSS_BITS * (p + 1) : 0u; }
__host__ __device__ constexpr uint32_t goss_width(uint32_t p) { return p + 1 < GOSS_PASSES ? GOSS_BITS : 64u - GOSS_BITS * (GOSS_PASSES - 1); }
static_assert(goss_shift(GOSS_PASSES - 2) == goss_width(GOSS_PASSES - 1) && goss_width(GOSS_PASSES - 1) <= GOSS_BITS, "the digits tile the 64 bits");

// FIRST: pass 0, which also gathers the keys.  root == nullptr: the list is the whole instance list; pos == nullptr: lam is in
// instance-list order already.  hist: [GOSS_PASSES][GOSS_BINS], zeroed before the chain.
template <bool FIRST>
__global__ __launch_bounds__(256) void goss_hist_kernel(const double* __restrict__ lam, const uint32_t* __restrict__ pos,
                                                        const uint32_t* __restrict__ root, uint32_t n, uint32_t pass,
                                                        const GossStateDev* __restrict__ st, unsigned long long* __restrict__ keys,
                                                        uint32_t* __restrict__ hist) {
    __shared__ uint32_t lh[GOSS_BINS];
    for (uint32_t t = threadIdx.x; t < GOSS_BINS; t += blockDim.x) lh[t] = 0u;
    __syncthreads();
    const uint32_t b = blockIdx.x * GOSS_SHARE, e = min(n, b + GOSS_SHARE);
    const uint32_t shift = goss_shift(pass), mask = (1u << goss_width(pass)) - 1u;
    const uint32_t above = FIRST ? 0u : goss_shift(pass - 1);  // (the bits above this digit: the prefix)
    const unsigned long long prefix = FIRST ? 0ull : st->prefix;
    for (uint32_t i = b + threadIdx.x; i < e; i += blockDim.x) {
        unsigned long long key;
        if (FIRST) {
            const uint32_t r = root ? root[i] : i;
            key = (unsigned long long)__double_as_longlong(fabs(lam[pos ? pos[r] : r]));
            keys[i] = key;
        } else {
            key = keys[i];
            if ((key >> above) != prefix) continue;
        }
        atomicAdd(&lh[(uint32_t)(key >> shift) & mask], 1u);
    }
    __syncthreads();
    uint32_t* out = hist + (size_t)pass * GOSS_BINS;
    for (uint32_t t = threadIdx.x; t < GOSS_BINS; t += blockDim.x)
        if (lh[t] != 0u) atomicAdd(&out[t], lh[t]);
}

// One wave.  Lane l owns the 32 digits GOSS_BINS - 1 - 32 l down to GOSS_BINS - 32 - 32 l; the lane whose digits hold the
// wanted rank walks them.  pass 0 starts from (prefix 0, rank n_top); 1 <= n_top <= the number of keys.
__global__ __launch_bounds__(64) void goss_pick_kernel(const uint32_t* __restrict__ hist, uint32_t pass, uint32_t n_top,
                                                       GossStateDev* __restrict__ st) {
    constexpr uint32_t PER = GOSS_BINS / 64;
    const uint32_t lane = threadIdx.x;
    const uint32_t* h = hist + (size_t)pass * GOSS_BINS;
    const uint32_t hi = GOSS_BINS - 1u - PER * lane;  // the lane's largest digit
    uint32_t own = 0;
    for (uint32_t j = 0; j < PER; j++) own += h[hi - j];
    uint32_t incl = own;  // inclusive sums over the lanes, i.e. over the digits from the largest down
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if ((int)lane >= o) incl += up;
    }
    const uint32_t k = pass == 0 ? n_top : st->rank;
    const unsigned long long prefix = pass == 0 ? 0ull : st->prefix;
    const uint32_t before = incl - own;
    if (before < k && k <= incl) {  // (exactly one lane: the sums are non-decreasing and the last one is >= k)
        uint32_t acc = before;
        for (uint32_t j = 0; j < PER; j++) {
            const uint32_t c = h[hi - j];
            if (acc + c >= k) {
                st->prefix = (prefix << goss_width(pass)) | (unsigned long long)(hi - j);
                st->rank = k - acc;
                break;
            }
            acc += c;
        }
    }
}

// flag[r] = 1 where the entry's key is tau (r: the entry's full-list index; entries outside the list are not written)
__global__ __launch_bounds__(256) void goss_tie_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ root,
                                                       uint32_t n, const GossStateDev* __restrict__ st, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[root ? root[i] : i] = keys[i] == st->prefix ? 1u : 0u;
}

__device__ __forceinline__ double goss_uniform(uint64_t key, uint32_t id) { return xe_gamma(key, id); }  // (the same counter-based stream)

// tie[r]: the exclusive prefix sums of goss_tie_kernel's flags.  top[r] = 1: a member of the top set; flag[r] = 1: kept.
// pos / perm: the entry's position and, by position, the document's original instance id.
__global__ __launch_bounds__(256) void goss_flag_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ root,
                                                        uint32_t n, const GossStateDev* __restrict__ st, const uint32_t* __restrict__ tie,
                                                        const uint32_t* __restrict__ pos, const uint32_t* __restrict__ perm,
                                                        unsigned long long tree_key, double p, uint8_t* __restrict__ top,
                                                        uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = root ? root[i] : i;
    const unsigned long long key = keys[i], tau = st->prefix;
    const bool is_top = key > tau || (key == tau && tie[r] < st->rank);
    const bool keep = is_top || goss_uniform(tree_key, perm[pos[r]]) < p;
    top[r] = is_top ? 1 : 0;
    flag[r] = keep ? 1u : 0u;
}

// hist_absmax_kernel over the GOSS list `root`, the kept others amplified
__global__ __launch_bounds__(256) void goss_absmax_kernel(const double* __restrict__ lam, const double* __restrict__ wt,
                                                          const uint32_t* __restrict__ pos, const uint32_t* __restrict__ root,
                                                          const uint8_t* __restrict__ top, double amp, uint32_t n,
                                                          unsigned long long* __restrict__ out /*[2]*/) {
    unsigned long long ml = 0, mw = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t r = root[i];
        const uint32_t p = pos ? pos[r] : r;
        const bool t = top[r] != 0;
        const double l = t ? lam[p] : lam[p] * amp, w = t ? wt[p] : wt[p] * amp;
        ml = max(ml, (unsigned long long)__double_as_longlong(fabs(l)));
        mw = max(mw, (unsigned long long)__double_as_longlong(fabs(w)));
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

// hist_quant_kernel over the GOSS list, the kept others amplified before the fixed-point step
__global__ __launch_bounds__(256) void goss_quant_kernel(const double* __restrict__ lam, const double* __restrict__ wt,
                                                         const uint32_t* __restrict__ pos, const uint32_t* __restrict__ root,
                                                         const uint8_t* __restrict__ top, double amp, uint32_t n, int s_l, int s_w,
                                                         int w_zero, long long* __restrict__ Q, long long* __restrict__ W) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = root[i];
    const uint32_t p = pos ? pos[r] : r;
    const bool t = top[r] != 0;
    const double l = t ? lam[p] : lam[p] * amp, w = t ? wt[p] : wt[p] * amp;
    Q[r] = (long long)rint(ldexp(l, s_l));
    W[r] = w_zero ? 0ll : (long long)rint(ldexp(w, s_w));
}
