// The arithmetic of a query's end in the bound-and-verify NDCG@k kernel (kernels_verify.inc) that the host can restate:
// the per-query gap bound of the rank walk and the division-free quotient dcg / norm.  One copy for the kernel, for the host
// that prepares the reciprocals (device_dataset.inc: upload_norms) and for the tests (fr_debug_verify_end), which hold both
// to the expressions they stand in for.  No HIP and no state here.
#pragma once
#include <cmath>
#include <cstddef>
#include <limits>

#if defined(__HIP__) || defined(__CUDACC__)
#define FR_VE_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define FR_VE_HD inline
#endif

namespace frdev {

// ---- the gap bound -------------------------------------------------------------------------------------------------
// verify_far(ka, kb) = (ka - kb) > fma(gam, |ka| + |kb|, eps0) decides a pair of sorted neighbours.  For a whole query one
// bound serves every pair: with B >= |k| for every key k the walk compares,
//     tau = fma(gam, 2 B, eps0) >= fma(gam, fl(|ka| + |kb|), eps0)
// because |ka| + |kb| <= 2 B in real numbers, 2 B is a double (or +inf) and rounding to nearest is monotone, so
// fl(|ka| + |kb|) <= 2 B; and fma(gam, x, eps0) is the rounding of a function that does not decrease in x while gam >= 0.
// Hence (ka - kb) > tau implies verify_far(ka, kb): the SAME rounded difference on the left, a right-hand side at least as
// large.  The converse does not hold and is not needed -- a pair the cheap test leaves open is decided by verify_far itself.
// The list is sorted (descending), so every compared key lies between the first and the last of them and
// B = max(|first|, |last|).  Whatever makes the bound meaningless makes the comparison false, which only sends the pair to
// verify_far: gam < 0 or NaN (tau = +inf / NaN), a key that is +-inf or NaN (B, hence tau, is inf or NaN), 2 B overflowing.
FR_VE_HD double verify_gap_bound(double first, double last, double gam, double eps0) {
    const double B = __builtin_fmax(__builtin_fabs(first), __builtin_fabs(last));  // (fmax drops a NaN: then the other key is
                                                                                  // NaN or the comparison against it false)
    const double tau = __builtin_fma(gam, B + B, eps0);
    return gam >= 0.0 ? tau : std::numeric_limits<double>::infinity();
}

// ---- the quotient --------------------------------------------------------------------------------------------------
// val = dcg / norm, correctly rounded, from rn = fl(1 / norm) (IEEE division on the host, once per query) and five FMAs:
//     q0 = fl(dcg rn)   r0 = fl(dcg - norm q0)   q1 = fl(q0 + r0 rn)   r1 = fl(dcg - norm q1)   val = fl(q1 + r1 rn)
// With u = 2^-53 and Q = dcg / norm: rn = (1 + e1) / norm, |e1| <= u, so q0 = Q (1 + e1)(1 + e2) is within (2 u + u^2) |Q|
// of Q; r0 = (dcg - norm q0)(1 + e3); before its rounding q1 is Q + (Q - q0) e with |e| <= 2 u + u^2, i.e. within
// 4.1 u^2 |Q| of Q -- far less than half the spacing of the doubles around Q (> u |Q| / 2) -- so q1 is one of the two doubles
// that enclose Q, or Q itself if Q is a double: a faithful quotient.  For a faithful q1 the residual dcg - norm q1 is a
// double (r1 is exact), and Markstein's theorem (IBM J. Res. Dev. 34, 1990; Muller et al., Handbook of Floating-Point
// Arithmetic, "Division": q faithful, y = RN(1 / b), r = a - b q exact  =>  RN(q + r y) = RN(a / b)) makes the last step the
// correctly rounded quotient -- the number the division gives, bit for bit.  The theorem needs every intermediate result
// to be a normal number (or an exact zero), which the ranges below give with a wide margin:
//     norm in [2^-256, 2^256]                  (verify_rnorm: anything else, 0 and NaN included, keeps the division)
//     dcg = 0 or 2^-112 <= |dcg| <= 2^205      (verify_terms_in_range over the dataset's term table: a sum of at most 20
//                                               terms, each 0 or of magnitude in [2^-60, 2^200], hence a multiple of 2^-112)
// so |Q| in [2^-368, 2^461] and r1, a multiple of ulp(norm) ulp(q1) >= 2^-728, cannot underflow.  dcg = +0 (the sum starts at
// +0.0 and never becomes -0.0) gives q0 = r0 = q1 = r1 = val = +0 = +0 / norm for norm > 0.  The bench's tables (five gain
// classes, terms 0 and 0.22 .. 15) and norms (0.28 .. 70) sit in the middle of these ranges.
constexpr double VERIFY_NORM_LO = 0x1p-256, VERIFY_NORM_HI = 0x1p256;
constexpr double VERIFY_TERM_LO = 0x1p-60, VERIFY_TERM_HI = 0x1p200;

FR_VE_HD double verify_quotient(double dcg, double norm, double rn) {
    const double q0 = dcg * rn;
    const double r0 = __builtin_fma(-norm, q0, dcg);
    const double q1 = __builtin_fma(r0, rn, q0);
    const double r1 = __builtin_fma(-norm, q1, dcg);
    return __builtin_fma(r1, rn, q1);
}

// what is uploaded beside norm: its reciprocal where verify_quotient is proven, NaN (= "divide") everywhere else
inline double verify_rnorm(double norm, bool terms_in_range) {
    return (terms_in_range && norm >= VERIFY_NORM_LO && norm <= VERIFY_NORM_HI) ? 1.0 / norm : std::numeric_limits<double>::quiet_NaN();
}

// every term of a dataset's DCG table is an exact zero or of magnitude in [VERIFY_TERM_LO, VERIFY_TERM_HI]
inline bool verify_terms_in_range(const double* tab, size_t n) {
    for (size_t i = 0; i < n; i++) {
        const double t = std::fabs(tab[i]);
        if (!(t == 0.0 || (t >= VERIFY_TERM_LO && t <= VERIFY_TERM_HI))) return false;
    }
    return true;
}

}  // namespace frdev
