// Interface between capi.cpp and normalize.hip (feature normalisation), and the arithmetic the two
// sides share: the statistics record of one feature (the reference's StreamingStats, src/stats.rs:53-104), its push, the
// fold of two records and the per-value functions (src/normalizers.rs:55-108).  tests/normalize_model.py restates all of it
// in numpy, operation for operation.  Everything here is compiled with -ffp-contract=off: no product meets its sum in an fma.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define FR_NORM_HD __host__ __device__
#else
#define FR_NORM_HD
#endif

namespace frdev {

constexpr uint32_t FR_STATS_CHUNK = 256;  // consecutive instances of the list one (chunk, feature) record is pushed over
constexpr uint32_t NORM_FEATS = 32;       // features of one workgroup of the statistics kernels: one word of the presence bits
constexpr uint32_t NORM_ROWS = 64;        // instances of one workgroup of normalize_apply_kernel
constexpr uint32_t NORM_COLS = 128;       // ... and its features
constexpr uint64_t NORM_NO_CELL = ~0ull;  // (instance << 32 | feature) of the lowest offending cell: none

struct NormRecord {
    uint64_t n;
    double mean, s, max, min, total;
};

FR_NORM_HD inline NormRecord norm_empty() { return NormRecord{0, 0.0, 0.0, -DBL_MAX, DBL_MAX, 0.0}; }

// src/stats.rs:67-90
FR_NORM_HD inline void norm_push(NormRecord& r, double x) {
    r.n += 1;
    const double old_mean = r.mean, old_s = r.s;
    if (r.max < x) r.max = x;
    if (r.min > x) r.min = x;
    r.total = r.total + x;
    if (r.n == 1) {
        r.mean = x;
        return;
    }
    const double dx = x - old_mean;
    r.mean = old_mean + dx / (double)r.n;
    const double dm = x - r.mean;
    r.s = old_s + dx * dm;
}

// a = a followed by b: an empty side leaves the other as it is
FR_NORM_HD inline void norm_fold(NormRecord& a, const NormRecord& b) {
    if (b.n == 0) return;
    if (a.n == 0) {
        a = b;
        return;
    }
    const uint64_t n = a.n + b.n;
    const double delta = b.mean - a.mean;
    const double share = (double)b.n / (double)n;
    const double mean = a.mean + delta * share;
    const double ss = a.s + b.s;
    const double d2 = delta * delta;
    const double nab = (double)a.n * (double)b.n;
    const double w = nab / (double)n;
    a.s = ss + d2 * w;
    a.mean = mean;
    a.total = a.total + b.total;
    if (a.max < b.max) a.max = b.max;
    if (a.min > b.min) a.min = b.min;
    a.n = n;
}

// what one value of a feature goes through: (val - a) / b in f32, or a constant, or nothing
enum NormKind : uint32_t { NORM_KEEP = 0, NORM_ZERO = 1, NORM_AFFINE = 2, NORM_SIGMOID = 3 };
struct NormParam {
    float a, b;
    uint32_t kind;
};

// src/normalizers.rs:57-63 (stddev_f32 = sqrt(variance) taken in f64, then cast) and :76-81
FR_NORM_HD inline NormParam norm_param_maxmin(double max, double min) {
    const float mx = (float)max, mn = (float)min;
    if (mx == mn) return NormParam{0.0f, 0.0f, NORM_ZERO};
    return NormParam{mn, mx - mn, NORM_AFFINE};
}
FR_NORM_HD inline NormParam norm_param_zscore(double mean, float stddev_f32) {
    if (stddev_f32 == 0.0f) return NormParam{0.0f, 0.0f, NORM_ZERO};
    return NormParam{(float)mean, stddev_f32, NORM_AFFINE};
}
FR_NORM_HD inline float norm_affine(float val, const NormParam& p) {
    const float num = val - p.a;
    return num / p.b;
}

enum NormMethod : int { NORM_M_ZSCORE = 0, NORM_M_MAXMIN = 1 };

// The documents of one dataset handle as the kernels visit them: the feature tiles (explain.hpp ExDocs) and, for every
// instance of the list in the view's iteration order, its padded position and its instance id.
struct NormDocs {
    const float* xb = nullptr;
    uint32_t dq = 0, d = 0;
    int device = 0;
    std::vector<uint32_t> pos, ids;
    const uint32_t* present = nullptr;  // the core's presence bits [instances][present_words], nullptr: every value is held
    size_t present_words = 0, core_n = 0;
    std::vector<uint32_t> fmask;        // [(d + 31) / 32] the features statistics are taken of
};

struct NormTimes {
    double kernel_ms = 0.0, copy_ms = 0.0;
};

// records[f] of every feature f < d over the list (chunk records, then the fold in chunk order); *bad = the lowest
// (instance << 32 | feature) among the held non-finite values of the masked features, NORM_NO_CELL when there is none
bool normalize_stats(const NormDocs& docs, std::vector<NormRecord>* records, uint64_t* bad, NormTimes* times, std::string* err);
// out[i * d + f] for the list's instance i (row-major, list order): params[f] applied to the held values, 0.0 for the
// absent ones; *bad = the lowest cell whose result is NaN
bool normalize_apply(const NormDocs& docs, const std::vector<NormParam>& params, float* out, uint64_t* bad, NormTimes* times, std::string* err);
// the same output under query scope: the list is qoff[q] .. qoff[q + 1] per query; *bad_stat = the lowest held non-finite
// cell (the statistics refuse it), *bad = the lowest NaN result.  out rows are indexed by docs.ids (unsampled: the list).
bool normalize_per_query(const NormDocs& docs, const std::vector<uint32_t>& qoff, int method, float* out, uint64_t* bad_stat, uint64_t* bad,
                         NormTimes* times, std::string* err);

}  // namespace frdev
