// Feature normalisation: per-feature statistics of a dataset or of every query, and the transform of
// the matrix.  A translation unit of its own, like explain.hip: device.o is built from its own sources and none of its
// kernels moves.  Four kernels:
//   stats_chunk_kernel      the record of every (chunk of 256 instances, feature): the reference's sequential push
//   stats_fold_kernel       one lane per feature folds the chunk records in chunk order
//   normalize_apply_kernel  applies one (a, b, kind) per feature and writes rows in instance order; flags the lowest NaN
//   normalize_query_kernel  a workgroup per (query, 32 features): the sequential push over the query, then the transform
// The arithmetic (push, fold, the per-value functions) is normalize.hpp's, shared with the host.
#include "normalize.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

namespace frdev {

#define NM_HIP(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            if (err) *err = std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr; \
            return false;                                                                   \
        }                                                                                   \
    } while (0)

namespace {

template <typename T>
struct NmBuf {
    T* p = nullptr;
    ~NmBuf() {
        if (p) (void)hipFree(p);
    }
    bool alloc(size_t n, std::string* err) {
        NM_HIP(hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)));
        return true;
    }
    bool upload(const T* v, size_t n, std::string* err) {
        if (!alloc(n, err)) return false;
        if (n) NM_HIP(hipMemcpy(p, v, n * sizeof(T), hipMemcpyHostToDevice));
        return true;
    }
    bool upload(const std::vector<T>& v, std::string* err) { return upload(v.data(), v.size(), err); }
};

struct NmTimer {
    hipEvent_t a = nullptr, b = nullptr;
    ~NmTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    bool begin(std::string* err) {
        if (!a) NM_HIP(hipEventCreate(&a));
        if (!b) NM_HIP(hipEventCreate(&b));
        NM_HIP(hipEventRecord(a, nullptr));
        return true;
    }
    bool end(double* ms_total, std::string* err) {
        NM_HIP(hipEventRecord(b, nullptr));
        NM_HIP(hipEventSynchronize(b));
        float ms = 0.0f;
        NM_HIP(hipEventElapsedTime(&ms, a, b));
        *ms_total += (double)ms;
        return true;
    }
};

// what every kernel here reads of a dataset
struct NmDocs {
    const float* xb;          // feature tiles (kernels_score.inc xb_index)
    const uint32_t* pos;      // [m] padded position of the list's instance i
    const uint32_t* ids;      // [m] its instance id
    const uint32_t* present;  // [core instances][pw] presence bits, nullptr: every value is held
    uint32_t dq, d, m, pw;
};

constexpr uint32_t NM_STRIDE = FR_STATS_CHUNK + 1;  // vals[feature][instance]: lanes = instances write, lanes = features read, no bank shared

// the 16 bytes of position p's features 4 * jq .. 4 * jq + 3
__device__ __forceinline__ float4 nm_quad(const float* xb, uint32_t p, uint32_t jq, uint32_t dq) {
    return *reinterpret_cast<const float4*>(xb + ((size_t)(p >> 6) * dq + jq) * 256 + (size_t)(p & 63) * 4);
}

// which of the features f0 .. f0 + 31 instance `id` holds (bit k: feature f0 + k; none at or past d)
__device__ __forceinline__ uint32_t nm_held(const NmDocs& a, uint32_t id, uint32_t g) {
    uint32_t bits = 0xFFFFFFFFu;
    if (a.present != nullptr) bits = g < a.pw ? a.present[(size_t)id * a.pw + g] : 0u;
    const uint32_t nf = a.d - g * NORM_FEATS;
    if (nf < NORM_FEATS) bits &= (1u << nf) - 1u;
    return bits;
}

// the two-branch form of src/normalizers.rs:112-120 in f64, rounded to f32 once
__device__ __forceinline__ float nm_sigmoid(float v) {
    const double x = (double)v;
    double r;
    if (x > 0.0) {
        const double z = exp(-x);
        r = 1.0 / (1.0 + z);
    } else {
        const double z = exp(x);
        r = z / (1.0 + z);
    }
    return (float)r;
}

__device__ __forceinline__ float nm_value(float v, const NormParam& p) {
    switch (p.kind) {
        case NORM_ZERO: return 0.0f;
        case NORM_AFFINE: return norm_affine(v, p);
        case NORM_SIGMOID: return nm_sigmoid(v);
        default: return v;
    }
}

__device__ __forceinline__ bool nm_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

__device__ __forceinline__ void nm_flag(unsigned long long* bad, uint32_t id, uint32_t f) {
    atomicMin(bad, ((unsigned long long)id << 32) | (unsigned long long)f);
}

// Stages instances base .. base + cnt of the list, features f0 .. f0 + 31: lane t = instance base + t loads its eight quads
// (16-byte reads of the tiles) into vals[feature][t] and its presence word into held[t]; a held non-finite value of a
// masked feature (fmask == nullptr: every feature) is flagged.
__device__ __forceinline__ void nm_stage(const NmDocs& a, uint32_t base, uint32_t cnt, uint32_t g, const uint32_t* fmask, unsigned long long* bad,
                                         float* vals, uint32_t* held, uint32_t* rowid) {
    const uint32_t t = threadIdx.x;
    if (t >= cnt) return;
    const uint32_t p = a.pos[base + t], id = a.ids[base + t];
    const uint32_t bits = nm_held(a, id, g);
    const uint32_t check = bits & (fmask != nullptr ? fmask[g] : 0xFFFFFFFFu);
    held[t] = bits;
    if (rowid != nullptr) rowid[t] = id;
    const uint32_t f0 = g * NORM_FEATS;
#pragma unroll
    for (uint32_t ql = 0; ql < NORM_FEATS / 4; ql++) {
        const uint32_t jq = (f0 >> 2) + ql;
        if (jq >= a.dq) break;
        const float4 v = nm_quad(a.xb, p, jq, a.dq);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t c = ql * 4 + k;
            vals[c * NM_STRIDE + t] = vv[k];
            if (((check >> c) & 1u) && !nm_finite(vv[k])) nm_flag(bad, id, f0 + c);
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// Dataset scope.  Workgroup (chunk, g): the chunk's 256 instances are staged, then lane k < 32 pushes the held values of
// feature 32 g + k in list order.  rec[chunk * d + f].
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stats_chunk_kernel(NmDocs a, const uint32_t* __restrict__ fmask, NormRecord* __restrict__ rec,
                                                          unsigned long long* __restrict__ bad) {
    __shared__ float vals[NORM_FEATS * NM_STRIDE];
    __shared__ uint32_t held[FR_STATS_CHUNK];
    const uint32_t chunk = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
    const uint32_t base = chunk * FR_STATS_CHUNK;
    const uint32_t cnt = a.m - base < FR_STATS_CHUNK ? a.m - base : FR_STATS_CHUNK;
    nm_stage(a, base, cnt, g, fmask, bad, vals, held, nullptr);
    __syncthreads();
    const uint32_t f = g * NORM_FEATS + t;
    if (t < NORM_FEATS && f < a.d) {
        NormRecord r = norm_empty();
        const float* col = vals + t * NM_STRIDE;
        for (uint32_t j = 0; j < cnt; j++)
            if ((held[j] >> t) & 1u) norm_push(r, (double)col[j]);
        rec[(size_t)chunk * a.d + f] = r;
    }
}

__global__ __launch_bounds__(64) void stats_fold_kernel(const NormRecord* __restrict__ rec, uint32_t chunks, uint32_t d, NormRecord* __restrict__ out) {
    const uint32_t f = blockIdx.x * 64 + threadIdx.x;
    if (f >= d) return;
    NormRecord acc = norm_empty();
    for (uint32_t c = 0; c < chunks; c++) norm_fold(acc, rec[(size_t)c * d + f]);
    out[f] = acc;
}

// ------------------------------------------------------------------------------------------------------------------
// Apply.  Workgroup (bx, by): instances 64 bx .. and features 128 by ..; lane = instance loads quads, the results pass
// through LDS so that the rows leave in 512-byte stretches.  out[i * d + f], i = place in the list.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void normalize_apply_kernel(NmDocs a, const NormParam* __restrict__ params, float* __restrict__ out,
                                                              unsigned long long* __restrict__ bad) {
    __shared__ float tile[NORM_ROWS * (NORM_COLS + 1)];
    const uint32_t t = threadIdx.x, r = t & 63u;
    const uint32_t i0 = blockIdx.x * NORM_ROWS, f0 = blockIdx.y * NORM_COLS;
    const uint32_t rows = a.m - i0 < NORM_ROWS ? a.m - i0 : NORM_ROWS;
    const uint32_t cols = a.d - f0 < NORM_COLS ? a.d - f0 : NORM_COLS;
    if (r < rows) {
        const uint32_t p = a.pos[i0 + r], id = a.ids[i0 + r];
        for (uint32_t ql = t >> 6; ql < NORM_COLS / 4; ql += 4) {
            const uint32_t jq = (f0 >> 2) + ql;
            if (jq >= a.dq) break;
            const uint32_t bits = nm_held(a, id, (f0 + ql * 4) / NORM_FEATS) >> ((ql * 4) & 31u);
            const float4 v = nm_quad(a.xb, p, jq, a.dq);
            const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t f = f0 + ql * 4 + k;
                if (f >= a.d) break;
                float res = 0.0f;
                if ((bits >> k) & 1u) {
                    res = nm_value(vv[k], params[f]);
                    if (res != res) nm_flag(bad, id, f);
                }
                tile[r * (NORM_COLS + 1) + ql * 4 + k] = res;
            }
        }
    }
    __syncthreads();
    for (uint32_t idx = t; idx < rows * cols; idx += 256) {
        const uint32_t rr = idx / cols, c = idx % cols;
        out[(size_t)(i0 + rr) * a.d + f0 + c] = tile[rr * (NORM_COLS + 1) + c];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Query scope.  Workgroup (q, g): the query's instances qoff[q] .. qoff[q + 1] of the list, 256 at a time through LDS;
// lane k < 32 keeps the record of feature 32 g + k in registers over all the blocks (the exact sequential push), finishes
// it (variance, square root and casts on the device) and leaves its (a, b, kind) in LDS; a second walk over the blocks
// transforms and writes out[id * d + f].  Fewer than two held values: 0.0.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void normalize_query_kernel(NmDocs a, const uint32_t* __restrict__ qoff, int method, float* __restrict__ out,
                                                              unsigned long long* __restrict__ bad_stat, unsigned long long* __restrict__ bad) {
    __shared__ float vals[NORM_FEATS * NM_STRIDE];
    __shared__ uint32_t held[FR_STATS_CHUNK];
    __shared__ uint32_t rowid[FR_STATS_CHUNK];
    __shared__ NormParam prm[NORM_FEATS];
    const uint32_t q = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
    const uint32_t b = qoff[q], e = qoff[q + 1];
    const uint32_t f0 = g * NORM_FEATS, f = f0 + t;
    const bool owner = t < NORM_FEATS && f < a.d;
    const uint32_t nf = a.d - f0 < NORM_FEATS ? a.d - f0 : NORM_FEATS;
    NormRecord r = norm_empty();
    for (uint32_t base = b; base < e; base += FR_STATS_CHUNK) {
        const uint32_t cnt = e - base < FR_STATS_CHUNK ? e - base : FR_STATS_CHUNK;
        nm_stage(a, base, cnt, g, nullptr, bad_stat, vals, held, nullptr);
        __syncthreads();
        if (owner) {
            const float* col = vals + t * NM_STRIDE;
            for (uint32_t j = 0; j < cnt; j++)
                if ((held[j] >> t) & 1u) norm_push(r, (double)col[j]);
        }
        __syncthreads();
    }
    if (owner) {
        NormParam p{0.0f, 0.0f, NORM_ZERO};
        if (r.n >= 2) {
            if (method == NORM_M_MAXMIN) {
                p = norm_param_maxmin(r.max, r.min);
            } else {
                const double var = r.s / (double)(r.n - 1);
                p = norm_param_zscore(r.mean, (float)__dsqrt_rn(var));
            }
        }
        prm[t] = p;
    }
    __syncthreads();
    for (uint32_t base = b; base < e; base += FR_STATS_CHUNK) {
        const uint32_t cnt = e - base < FR_STATS_CHUNK ? e - base : FR_STATS_CHUNK;
        nm_stage(a, base, cnt, g, nullptr, bad_stat, vals, held, rowid);
        __syncthreads();
        for (uint32_t idx = t; idx < cnt * nf; idx += 256) {
            const uint32_t rr = idx / nf, c = idx % nf;
            float res = 0.0f;
            if ((held[rr] >> c) & 1u) {
                res = nm_value(vals[c * NM_STRIDE + rr], prm[c]);
                if (res != res) nm_flag(bad, rowid[rr], f0 + c);
            }
            out[(size_t)rowid[rr] * a.d + f0 + c] = res;
        }
        __syncthreads();
    }
}

namespace {

struct NmDevice {
    NmBuf<uint32_t> pos, ids, present, fmask;
    NmBuf<unsigned long long> bad;  // [2]
    NmDocs a{};
    bool upload(const NormDocs& docs, std::string* err) {
        if (docs.pos.size() != docs.ids.size() || docs.pos.size() > 0xFFFFFF00u || docs.d == 0) {
            if (err) *err = "normalisation: bad document list";
            return false;
        }
        if (docs.present != nullptr)
            for (uint32_t id : docs.ids)
                if (id >= docs.core_n) {
                    if (err) *err = "normalisation: an instance outside the presence bits";
                    return false;
                }
        if (!pos.upload(docs.pos, err) || !ids.upload(docs.ids, err)) return false;
        if (docs.present != nullptr && !present.upload(docs.present, docs.core_n * docs.present_words, err)) return false;
        if (!docs.fmask.empty() && !fmask.upload(docs.fmask, err)) return false;
        const unsigned long long none[2] = {NORM_NO_CELL, NORM_NO_CELL};
        if (!bad.upload(none, 2, err)) return false;
        a.xb = docs.xb, a.pos = pos.p, a.ids = ids.p, a.present = docs.present != nullptr ? present.p : nullptr;
        a.dq = docs.dq, a.d = docs.d, a.m = (uint32_t)docs.pos.size(), a.pw = (uint32_t)docs.present_words;
        return true;
    }
    bool flags(uint64_t* first, uint64_t* second, std::string* err) {
        unsigned long long h[2];
        NM_HIP(hipMemcpy(h, bad.p, sizeof(h), hipMemcpyDeviceToHost));
        if (first) *first = h[0];
        if (second) *second = h[1];
        return true;
    }
};

// device rows [n][d] -> host, through two page-locked slabs (pageable memory when there is none left)
bool nm_download(const float* dev, float* host, size_t n, size_t d, std::string* err) {
    const size_t row = d * sizeof(float), total = n * row;
    if (total == 0) return true;
    const size_t slab = std::min<size_t>(total, (size_t)32 << 20);
    float* pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    const bool pinned = hipHostMalloc((void**)&pin[0], slab, hipHostMallocDefault) == hipSuccess &&
                        hipHostMalloc((void**)&pin[1], slab, hipHostMallocDefault) == hipSuccess &&
                        hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    auto release = [&]() {
        for (int k = 0; k < 2; k++) {
            if (pin[k]) (void)hipHostFree(pin[k]);
            if (ev[k]) (void)hipEventDestroy(ev[k]);
        }
    };
    if (!pinned) {
        (void)hipGetLastError();
        release();
        NM_HIP(hipMemcpy(host, dev, total, hipMemcpyDeviceToHost));
        return true;
    }
    const char* src = (const char*)dev;
    char* dst = (char*)host;
    size_t off[2] = {0, 0}, len[2] = {0, 0};
    hipError_t bad = hipSuccess;
    int turn = 0;
    for (size_t at = 0; at < total && bad == hipSuccess; at += slab, turn ^= 1) {
        if (len[turn]) {  // (this slab's previous copy has to land before it is reused)
            bad = hipEventSynchronize(ev[turn]);
            if (bad == hipSuccess) std::memcpy(dst + off[turn], pin[turn], len[turn]);
        }
        off[turn] = at, len[turn] = std::min(slab, total - at);
        if (bad == hipSuccess) bad = hipMemcpyAsync(pin[turn], src + at, len[turn], hipMemcpyDeviceToHost, nullptr);
        if (bad == hipSuccess) bad = hipEventRecord(ev[turn], nullptr);
    }
    for (int k = 0; k < 2 && bad == hipSuccess; k++, turn ^= 1) {
        if (!len[turn]) continue;
        bad = hipEventSynchronize(ev[turn]);
        if (bad == hipSuccess) std::memcpy(dst + off[turn], pin[turn], len[turn]);
    }
    if (bad != hipSuccess) (void)hipDeviceSynchronize();
    release();
    NM_HIP(bad);
    return true;
}

}  // namespace

bool normalize_stats(const NormDocs& docs, std::vector<NormRecord>* records, uint64_t* bad, NormTimes* times, std::string* err) {
    records->assign(docs.d, norm_empty());
    if (bad) *bad = NORM_NO_CELL;
    if (docs.pos.empty()) return true;
    NM_HIP(hipSetDevice(docs.device));
    NmDevice dev;
    if (!dev.upload(docs, err)) return false;
    if (docs.fmask.size() != (docs.d + 31) / 32) {
        if (err) *err = "normalisation: the feature mask does not cover the matrix";
        return false;
    }
    const uint32_t chunks = (dev.a.m + FR_STATS_CHUNK - 1) / FR_STATS_CHUNK, groups = (docs.d + NORM_FEATS - 1) / NORM_FEATS;
    if (groups > 65535u) {
        if (err) *err = "normalisation: too many features for one launch";
        return false;
    }
    NmBuf<NormRecord> rec, folded;
    if (!rec.alloc((size_t)chunks * docs.d, err) || !folded.alloc(docs.d, err)) return false;
    NormTimes scratch;
    NormTimes* tt = times ? times : &scratch;
    NmTimer tm;
    if (!tm.begin(err)) return false;
    stats_chunk_kernel<<<dim3(chunks, groups), 256>>>(dev.a, dev.fmask.p, rec.p, dev.bad.p);
    NM_HIP(hipGetLastError());
    stats_fold_kernel<<<(docs.d + 63) / 64, 64>>>(rec.p, chunks, docs.d, folded.p);
    NM_HIP(hipGetLastError());
    if (!tm.end(&tt->kernel_ms, err)) return false;
    NM_HIP(hipMemcpy(records->data(), folded.p, (size_t)docs.d * sizeof(NormRecord), hipMemcpyDeviceToHost));
    return dev.flags(bad, nullptr, err);
}

bool normalize_apply(const NormDocs& docs, const std::vector<NormParam>& params, float* out, uint64_t* bad, NormTimes* times, std::string* err) {
    if (bad) *bad = NORM_NO_CELL;
    if (docs.pos.empty()) return true;
    if (params.size() != docs.d) {
        if (err) *err = "normalisation: one parameter record per matrix column is needed";
        return false;
    }
    NM_HIP(hipSetDevice(docs.device));
    NmDevice dev;
    if (!dev.upload(docs, err)) return false;
    const uint32_t bx = (dev.a.m + NORM_ROWS - 1) / NORM_ROWS, by = (docs.d + NORM_COLS - 1) / NORM_COLS;
    if (by > 65535u) {
        if (err) *err = "normalisation: too many features for one launch";
        return false;
    }
    NmBuf<NormParam> prm;
    NmBuf<float> res;
    if (!prm.upload(params, err) || !res.alloc((size_t)dev.a.m * docs.d, err)) return false;
    NormTimes scratch;
    NormTimes* tt = times ? times : &scratch;
    NmTimer tm;
    if (!tm.begin(err)) return false;
    normalize_apply_kernel<<<dim3(bx, by), 256>>>(dev.a, prm.p, res.p, dev.bad.p);
    NM_HIP(hipGetLastError());
    if (!tm.end(&tt->kernel_ms, err)) return false;
    if (!dev.flags(bad, nullptr, err)) return false;
    if (bad && *bad != NORM_NO_CELL) return true;  // (refused: nothing is brought back)
    if (!tm.begin(err) || !nm_download(res.p, out, dev.a.m, docs.d, err) || !tm.end(&tt->copy_ms, err)) return false;
    return true;
}

bool normalize_per_query(const NormDocs& docs, const std::vector<uint32_t>& qoff, int method, float* out, uint64_t* bad_stat, uint64_t* bad,
                         NormTimes* times, std::string* err) {
    if (bad) *bad = NORM_NO_CELL;
    if (bad_stat) *bad_stat = NORM_NO_CELL;
    if (docs.pos.empty() || qoff.size() < 2) return true;
    if (qoff.back() != docs.pos.size()) {
        if (err) *err = "normalisation: the query offsets do not cover the document list";
        return false;
    }
    for (uint32_t id : docs.ids)  // (the rows go to out[id]: the list is a whole dataset's)
        if (id >= docs.ids.size()) {
            if (err) *err = "normalisation: query scope takes an unsampled dataset";
            return false;
        }
    NM_HIP(hipSetDevice(docs.device));
    NmDevice dev;
    if (!dev.upload(docs, err)) return false;
    const uint32_t groups = (docs.d + NORM_FEATS - 1) / NORM_FEATS;
    if (groups > 65535u) {
        if (err) *err = "normalisation: too many features for one launch";
        return false;
    }
    NmBuf<uint32_t> qo;
    NmBuf<float> res;
    if (!qo.upload(qoff, err) || !res.alloc((size_t)dev.a.m * docs.d, err)) return false;
    NormTimes scratch;
    NormTimes* tt = times ? times : &scratch;
    NmTimer tm;
    if (!tm.begin(err)) return false;
    normalize_query_kernel<<<dim3((uint32_t)qoff.size() - 1, groups), 256>>>(dev.a, qo.p, method, res.p, dev.bad.p, dev.bad.p + 1);
    NM_HIP(hipGetLastError());
    if (!tm.end(&tt->kernel_ms, err)) return false;
    if (!dev.flags(bad_stat, bad, err)) return false;
    if ((bad_stat && *bad_stat != NORM_NO_CELL) || (bad && *bad != NORM_NO_CELL)) return true;
    if (!tm.begin(err) || !nm_download(res.p, out, dev.a.m, docs.d, err) || !tm.end(&tt->copy_ms, err)) return false;
    return true;
}

}  // namespace frdev
