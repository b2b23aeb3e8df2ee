// The evaluation measures in one place, host only (no HIP): the table of accepted names with their
// cut-off rules, the per-query norms the two metric kernels are handed, the measures themselves in scalar form over a
// ranked list, and the rule that routes a size class to the selection kernel.  make_evaluator (host.hpp) resolves a name
// through resolve(); metric_sort_kernel (kernels_metric.inc) and metric_topk_kernel (kernels_metric_topk.inc) implement
// the scalar definitions below with the same operands in the same order; tests/measures_host_sanitize.cpp runs this file
// under the sanitizers.
//
// A ranked list r = 1..n is a query's documents in the reference order (score descending, then the layout's position).
// rel_r means gain_r > 0, gexp_r = 2^gain_r - 1, L = min(k, n) with a cut-off k and n without.  Every sum is a sequential
// f64 sum from 0.0 in rank order, unfused.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace frmeasure {

// (the values of frdev::Measure, device.hpp; host.hpp asserts that the two agree)
enum : int { NDCG = 0, AP = 1, RR = 2, DCG = 3, PRECISION = 4, RECALL = 5, SUCCESS = 6, ERR = 7, MEASURE_COUNT = 8 };

enum Cutoff : int { CUT_OPTIONAL = 0, CUT_REQUIRED = 1, CUT_IGNORED = 2 };

struct MeasureInfo {
    int id;
    const char* display;    // Evaluator::name without its "@k"
    Cutoff cutoff;
    const char* names[2];   // lower case; names[0] is the one measures() lists first, names[1] an alias or nullptr
};

// "p" is not an alias of precision: "p@5" stays an invalid measure, as the C ABI's tests pin it.
inline const MeasureInfo* measure_table() {
    static const MeasureInfo t[MEASURE_COUNT] = {
        {NDCG, "NDCG", CUT_OPTIONAL, {"ndcg", nullptr}},
        {AP, "AP", CUT_IGNORED, {"map", "ap"}},
        {RR, "RR", CUT_IGNORED, {"mrr", "rr"}},
        {DCG, "DCG", CUT_OPTIONAL, {"dcg", nullptr}},
        {PRECISION, "Precision", CUT_REQUIRED, {"precision", "prec"}},
        {RECALL, "Recall", CUT_OPTIONAL, {"recall", nullptr}},
        {SUCCESS, "Success", CUT_REQUIRED, {"success", nullptr}},
        {ERR, "ERR", CUT_OPTIONAL, {"err", nullptr}},
    };
    return t;
}

inline const char* cutoff_name(Cutoff c) { return c == CUT_OPTIONAL ? "optional" : c == CUT_REQUIRED ? "required" : "ignored"; }

inline const MeasureInfo* find_measure(const std::string& lower_name) {
    const MeasureInfo* t = measure_table();
    for (int i = 0; i < MEASURE_COUNT; i++)
        for (const char* nm : t[i].names)
            if (nm != nullptr && lower_name == nm) return &t[i];
    return nullptr;
}

// one of the five measures that came after NDCG, AP and RR
inline bool is_cut_measure(int measure) { return measure >= DCG && measure <= ERR; }

struct Resolved {
    int measure = NDCG;
    std::string display;  // "NDCG@10", "AP", "Precision@5", ...
};

// `lower_name`: the text before the '@', lower-cased; depth: the number after it, or -1 without one.  False with an empty
// *err: no such measure (the caller words that refusal, with the text the user gave); false with a text: a cut-off rule.
inline bool resolve(const std::string& lower_name, int64_t depth, Resolved* out, std::string* err) {
    err->clear();
    const MeasureInfo* mi = find_measure(lower_name);
    if (mi == nullptr) return false;
    if (mi->cutoff == CUT_REQUIRED && depth < 0) {
        *err = std::string(mi->display) + " needs a cut-off: write \"" + mi->names[0] + "@k\" with k >= 1, not \"" + lower_name + "\"";
        return false;
    }
    if (mi->cutoff == CUT_REQUIRED && depth == 0) {
        *err = std::string(mi->display) + " needs a cut-off of at least 1: \"" + lower_name + "@0\" divides by nothing";
        return false;
    }
    out->measure = mi->id;
    out->display = mi->display;
    if (mi->cutoff != CUT_IGNORED && depth >= 0) out->display += "@" + std::to_string(depth);
    return true;
}

// ---- norms: what a query's entry of the kernels' `norms` array holds ----------------------------------------------------
//   NDCG       the ideal DCG (host.hpp), NaN for a query without a relevant document
//   AP, RECALL the number of relevant documents: of the judgments when the query is judged, else of the dataset; 0 makes
//              the kernel fall back to the ranked list's own count
//   PRECISION  the cut-off k as a double: the value divides by k, not by L
//   ERR        den = 2^gmax, the same for every query
//   RR, DCG, SUCCESS  unused (0)

template <class It>
inline uint32_t count_relevant(It first, It last) {
    uint32_t c = 0;
    for (; first != last; ++first) c += *first > 0.0f;
    return c;
}

// gmax: the largest gain of the dataset's CORE (and of every judgment, with judgments), floored at 0.
inline float gmax_of(const float* gains, size_t n, float start = 0.0f) {
    float g = start > 0.0f ? start : 0.0f;
    for (size_t i = 0; i < n; i++)
        if (gains[i] > g) g = gains[i];
    return g;
}

// den = 2^gmax with the platform libm, as gexp = 2^gain - 1 is computed.  A power of two for integer gains, so that
// R = gexp / den is exact.
inline bool err_den(float gmax, double* den, std::string* err) {
    const double d = std::pow(2.0, (double)(gmax > 0.0f ? gmax : 0.0f));
    if (!std::isfinite(d)) {
        *err = "ERR: the largest gain " + std::to_string(gmax) + " gives no finite 2^gain to divide by";
        return false;
    }
    *den = d;
    return true;
}

// ---- the measures over a ranked list -----------------------------------------------------------------------------------

inline size_t cut_len(size_t n, int64_t depth) { return depth >= 0 && (uint64_t)depth < n ? (size_t)depth : n; }

inline double discount(size_t rank0) { return std::log2((double)rank0 + 2.0); }  // the kernels' disc[rank0]

inline double dcg_at(const double* gexp, size_t n, int64_t depth) {
    const size_t L = cut_len(n, depth);
    double dcg = 0.0;
    for (size_t i = 0; i < L; i++) dcg = dcg + gexp[i] / discount(i);
    return dcg;
}

inline uint32_t relevant_at(const float* gain, size_t n, int64_t depth) {
    return count_relevant(gain, gain + cut_len(n, depth));
}

// k_norm: the PRECISION norm, (double)k
inline double precision_at(const float* gain, size_t n, int64_t depth, double k_norm) {
    return (double)relevant_at(gain, n, depth) / k_norm;
}

// norm: the RECALL norm (a count; 0: the whole list's own)
inline double recall_at(const float* gain, size_t n, int64_t depth, double norm) {
    uint32_t num_rel = (uint32_t)norm;
    if (num_rel == 0) num_rel = relevant_at(gain, n, -1);
    return num_rel != 0 ? (double)relevant_at(gain, n, depth) / (double)num_rel : 0.0;
}

inline double success_at(const float* gain, size_t n, int64_t depth) { return relevant_at(gain, n, depth) != 0 ? 1.0 : 0.0; }

inline double err_at(const float* gain, const double* gexp, size_t n, int64_t depth, double den) {
    const size_t L = cut_len(n, depth);
    double p = 1.0, e = 0.0;
    for (size_t i = 0; i < L; i++) {
        const double R = gain[i] > 0.0f ? gexp[i] / den : 0.0;
        e = e + (p * R) / (double)(i + 1);
        p = p * (1.0 - R);
    }
    return e;
}

// any of the five by id; gexp may be null for the measures that do not read it
inline double cut_measure_at(int measure, const float* gain, const double* gexp, size_t n, int64_t depth, double norm) {
    switch (measure) {
        case DCG: return dcg_at(gexp, n, depth);
        case PRECISION: return precision_at(gain, n, depth, norm);
        case RECALL: return recall_at(gain, n, depth, norm);
        case SUCCESS: return success_at(gain, n, depth);
        case ERR: return err_at(gain, gexp, n, depth, norm);
        default: return std::nan("");
    }
}

// ---- routing -----------------------------------------------------------------------------------------------------------
// metric_topk_kernel can take a measure at all: one of the five, with a cut-off whose winners fit a wave's lanes.
constexpr int64_t TOPK_MAX_DEPTH = 64;
inline bool metric_topk_legal(int measure, int64_t depth, bool want_rank) {
    return is_cut_measure(measure) && depth >= 1 && depth <= TOPK_MAX_DEPTH && !want_rank;
}

// Does selection pay for a size class of npad (a power of two >= 64) documents at this depth?  By operation counts a wave
// selects with depth * npad / 64 key visits per lane and 6 depth cross-lane steps, against the sort network's
// npad / 2 * log2(npad) (log2(npad) + 1) / 2 compare-exchanges per block with a barrier after each of its
// log2(npad) (log2(npad) + 1) / 2 stages: selection is linear in the depth, the sort all but flat in it, so each class has a
// depth up to which selection wins.  Those depths are set from tools/metricbench.py's table at the 30K shape (DESIGN.md
// section 17: depths 1, 10, 20, 64; dcg and err; 1 and 64 slots): the largest measured depth at which the selection kernel's
// slowest run lay below the sort kernel's fastest for both measures and both slot counts.  Classes of 2048 .. 8192 do not
// occur in that shape and take the 1024 class's depth (selection gains on the sort with the length); from 16384 on the sort
// runs in a global scratch slab, which selection does not need at all.
constexpr uint32_t TOPK_ALWAYS_FROM_NPAD = 16384;
inline int64_t metric_topk_max_depth(uint32_t npad) {
    if (npad >= TOPK_ALWAYS_FROM_NPAD) return TOPK_MAX_DEPTH;
    if (npad == 256 || npad == 512) return 20;
    return 10;
}
inline bool metric_topk_pays(int64_t depth, uint32_t npad) {
    if (depth < 1 || depth > TOPK_MAX_DEPTH || npad == 0) return false;
    return depth <= metric_topk_max_depth(npad);
}

}  // namespace frmeasure
