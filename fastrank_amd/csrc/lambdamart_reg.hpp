// LambdaMART's leaf regularisation, host side ("Leaf regularisation"; device side: kernels_histreg.inc).
//
// Pure functions: no HIP, no environment.  For a node or candidate side with integer sums (Q, W), n instances, parent
// output p (none for the root) and interval [lo, hi] (the whole line without monotone signs), with G = ldexp(Q, -s_l),
// H = ldexp(W, -s_w) and den = H + lambda_l2, every operation f64 and rounded on its own:
//   1. T  = G > l1 ? G - l1 : (G < -l1 ? G + l1 : 0.0)
//   2. q0 = T / den, 0.0 when den == 0
//   3. o  = q0, clipped to [-mds, +mds] when max_delta_step > 0
//   4. with path_smooth > 0 and a parent: r = (double)n / path_smooth, o = (o r) / (r + 1.0) + p / (r + 1.0)
//   5. v  = o clamped to [lo, hi]
//   6. term = v == q0 ? (T T) / den : (2.0 T) v - (den v) v
// The scan kernels compute the same with selects; HistGrower uses these for a node's own term, the children's outputs and
// intervals and the leaf values whenever one of the three keys is set.
#pragma once
#include <cmath>
#include <cstdint>

namespace fr {

// the three numbers (all 0: off, and none of this header is used)
struct HistReg {
    double lambda_l1 = 0.0, max_delta_step = 0.0, path_smooth = 0.0;
    bool on() const { return lambda_l1 != 0.0 || max_delta_step != 0.0 || path_smooth != 0.0; }
};

// what steps 1 and 2 leave of an integer pair
struct RegSums {
    double T, den, q0;
};
// an output and its term
struct RegSide {
    double v, term;
};

inline double reg_threshold(double g, double l1) { return g > l1 ? g - l1 : (g < -l1 ? g + l1 : 0.0); }

inline RegSums reg_sums(long long q, long long w, int s_l, int s_w, double l1, double l2) {
    const double T = reg_threshold(std::ldexp((double)q, -s_l), l1), den = std::ldexp((double)w, -s_w) + l2;
    return {T, den, den != 0.0 ? T / den : 0.0};
}

// steps 3 to 5 from q0
inline double reg_output(double q0, uint32_t n, const HistReg& reg, const double* parent, double lo, double hi) {
    double o = q0;
    if (reg.max_delta_step > 0.0) {
        o = o > reg.max_delta_step ? reg.max_delta_step : o;
        o = o < -reg.max_delta_step ? -reg.max_delta_step : o;
    }
    if (reg.path_smooth > 0.0 && parent != nullptr) {
        const double r = (double)n / reg.path_smooth;
        o = (o * r) / (r + 1.0) + *parent / (r + 1.0);
    }
    const double v = o < lo ? lo : o;
    return v > hi ? hi : v;
}

// step 6 at a given output
inline double reg_term_at(const RegSums& s, double v) { return v == s.q0 ? (s.T * s.T) / s.den : (2.0 * s.T) * v - (s.den * v) * v; }

// steps 1 to 6 (parent == nullptr: the root, step 4 skipped)
inline RegSide reg_side(long long q, long long w, uint32_t n, int s_l, int s_w, double l2, const HistReg& reg, const double* parent, double lo,
                        double hi) {
    const RegSums s = reg_sums(q, w, s_l, s_w, reg.lambda_l1, l2);
    const double v = reg_output(s.q0, n, reg, parent, lo, hi);
    return {v, reg_term_at(s, v)};
}

// a node's own term at its carried output
inline double reg_own_term(long long q, long long w, int s_l, int s_w, double l2, const HistReg& reg, double v_node) {
    return reg_term_at(reg_sums(q, w, s_l, s_w, reg.lambda_l1, l2), v_node);
}

}  // namespace fr
