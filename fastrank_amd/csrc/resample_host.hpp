// Host side of model comparison: the options, the refusals, the fixed-shape sum, and the report made
// of the bootstrap and permutation arrays the device returns (resample.hpp states both).  No HIP, no environment.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "host.hpp"
#include "resample.hpp"

namespace fr {

struct ResampleOptions {
    uint32_t trials = 10000;
    uint64_t seed = 0;
    double alpha = 0.05;
};

// {"trials", "seed", "alpha"}, each optional; any other key is refused by name
inline ResampleOptions resample_options_from_json(const Value& v) {
    if (!v.is_object()) fail_raw("Error(\"invalid type: expected a map for the resampling options\", line: 0, column: 0)");
    ResampleOptions o;
    for (const auto& kv : v.obj) {
        if (kv.first == "trials") {
            const uint64_t t = json_u64(kv.second, "trials");
            if (t < 1 || t > frresample::MAX_TRIALS)
                fail_str("invalid value: trials must be between 1 and " + std::to_string(frresample::MAX_TRIALS) + ", not " + std::to_string(t));
            o.trials = (uint32_t)t;
        } else if (kv.first == "seed") {
            o.seed = json_u64(kv.second, "seed");
        } else if (kv.first == "alpha") {
            o.alpha = json_f64(kv.second, "alpha");
            if (!(o.alpha > 0.0 && o.alpha < 1.0)) fail_str("invalid value: alpha must lie strictly between 0 and 1");
        } else {
            fail_raw("Error(\"unknown field `" + kv.first + "`, expected one of `trials`, `seed`, `alpha`\", line: 0, column: 0)");
        }
    }
    return o;
}

// the limits of the table, and every value finite: the message names the row and the column
inline void resample_check(const double* V, size_t Q, size_t M) {
    if (M < 1 || M > frresample::MAX_SYSTEMS)
        fail_str("invalid value: a comparison takes between 1 and " + std::to_string(frresample::MAX_SYSTEMS) + " systems, not " + std::to_string(M));
    if (Q < 1) fail_str("invalid value: a comparison needs at least one query");
    if (Q > 0xFFFFFFFFull) fail_str("invalid value: a comparison takes fewer than 2^32 queries");
    if (!V) fail_str("NULL pointer: values");
    for (size_t q = 0; q < Q; q++)
        for (size_t c = 0; c < M; c++)
            if (!std::isfinite(V[q * M + c]))
                fail_str("non-finite value in row " + std::to_string(q) + ", column " + std::to_string(c) + ": resampling needs finite values");
}

// SUM of x[0], x[stride], ..: segments of frresample::SEG terms added one after the other from +0.0, the partials likewise
inline double resample_sum(const double* x, size_t n, size_t stride) {
    double total = 0.0;
    for (size_t s0 = 0; s0 < n; s0 += frresample::SEG) {
        const size_t s1 = std::min<size_t>(n, s0 + frresample::SEG);
        double part = 0.0;
        for (size_t i = s0; i < s1; i++) part += x[i * stride];
        total += part;
    }
    return total;
}

// src/stats.rs:142-155 PercentileStats::percentile over ascending data, as written: the weight `interp` (the fractional part
// of the position) multiplies the LOWER order statistic and 1 - interp the upper one, so the nearer of the two weighs less.
inline double resample_percentile(const std::vector<double>& sorted, double percentile) {
    const double n = percentile * (double)(sorted.size() - 1);
    const size_t lhs = (size_t)std::trunc(n);
    const size_t rhs = std::min(sorted.size(), (size_t)std::ceil(n));
    const double interp = n - std::trunc(n);
    if (lhs == rhs) return sorted[lhs];
    return (interp * sorted[lhs]) + (1.0 - interp) * sorted[rhs];
}

// the interval at level 1 - alpha of ascending data: order statistics, no interpolation
inline std::pair<double, double> resample_interval(const std::vector<double>& sorted, double alpha) {
    const double last = (double)(sorted.size() - 1);
    const size_t lo = (size_t)std::floor(alpha / 2.0 * last);
    const size_t hi = std::min(sorted.size() - 1, (size_t)std::ceil((1.0 - alpha / 2.0) * last));
    return {sorted[lo], sorted[hi]};
}

// The report of V[Q][M] and the device's arrays boot / perm (T x M each; either may be null: its parts are left out):
//   means[c] = SUM_q V[q][c] / Q;  intervals[c], summary[c] (p5 p25 p50 p75 p95) from the sorted boot[.][c]
//   pairs, i < j: diff = means[i] - means[j]; diff_interval from the sorted boot[t][i] - boot[t][j]; wins / losses / ties =
//   the queries where i is above / below / equal to j; p = (1 + #{t : range[t] >= |diff|}) / (T + 1), range[t] = max_c
//   perm[t][c] - min_c perm[t][c] (the randomised Tukey HSD test; exact f64 comparisons)
inline Value resample_report(const double* V, size_t Q, size_t M, size_t T, double alpha, const double* boot, const double* perm) {
    Value out = Value::object();
    std::vector<double> means(M);
    Value jm = Value::array();
    for (size_t c = 0; c < M; c++) {
        means[c] = resample_sum(V + c, Q, M) / (double)Q;
        jm.push(Value::number(means[c]));
    }
    out.set("means", jm);
    auto pair_of = [](const std::pair<double, double>& iv) {
        Value a = Value::array();
        a.push(Value::number(iv.first)), a.push(Value::number(iv.second));
        return a;
    };
    std::vector<double> col(boot ? T : 0);
    if (boot) {
        Value ji = Value::array(), js = Value::array();
        for (size_t c = 0; c < M; c++) {
            for (size_t t = 0; t < T; t++) col[t] = boot[t * M + c];
            std::sort(col.begin(), col.end());
            ji.push(pair_of(resample_interval(col, alpha)));
            Value s = Value::object();
            const char* names[5] = {"p5", "p25", "p50", "p75", "p95"};
            const double at[5] = {0.05, 0.25, 0.5, 0.75, 0.95};
            for (int k = 0; k < 5; k++) s.set(names[k], Value::number(resample_percentile(col, at[k])));
            js.push(s);
        }
        out.set("intervals", ji), out.set("summary", js);
    }
    std::vector<double> range(perm ? T : 0);
    for (size_t t = 0; perm && t < T; t++) {
        double lo = perm[t * M], hi = perm[t * M];
        for (size_t c = 1; c < M; c++) lo = std::min(lo, perm[t * M + c]), hi = std::max(hi, perm[t * M + c]);
        range[t] = hi - lo;
    }
    Value jp = Value::array();
    for (size_t i = 0; i < M; i++)
        for (size_t j = i + 1; j < M; j++) {
            Value p = Value::object();
            const double diff = means[i] - means[j];
            p.set("i", Value::uint(i)), p.set("j", Value::uint(j)), p.set("diff", Value::number(diff));
            if (boot) {
                for (size_t t = 0; t < T; t++) col[t] = boot[t * M + i] - boot[t * M + j];
                std::sort(col.begin(), col.end());
                p.set("diff_interval", pair_of(resample_interval(col, alpha)));
            }
            if (perm) {
                uint64_t count = 0;
                for (size_t t = 0; t < T; t++) count += range[t] >= std::fabs(diff) ? 1 : 0;
                p.set("p", Value::number((double)(1 + count) / (double)(T + 1)));
            }
            uint64_t wins = 0, losses = 0, ties = 0;
            for (size_t q = 0; q < Q; q++) {
                const double a = V[q * M + i], b = V[q * M + j];
                wins += a > b, losses += a < b, ties += a == b;
            }
            p.set("wins", Value::uint(wins)), p.set("losses", Value::uint(losses)), p.set("ties", Value::uint(ties));
            jp.push(p);
        }
    out.set("pairs", jp);
    return out;
}

}  // namespace fr
