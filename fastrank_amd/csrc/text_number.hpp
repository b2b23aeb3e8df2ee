// The fast grammar and value rule of the device text parser ("Text loading"), in plain C++ that compiles for
// the host and for the device: kernels_text.inc runs it per token, fr_debug_text_number runs the host compile of the same
// lines, and tests/ranksvm_text_cases.py restates it in Python.
//
// A fast number is [-+]?digits*(.digits*)?([eE][-+]?digits)? with at least one mantissa digit, at most 19 significant
// digits after leading zeros (so m < 10^19 < 2^64) and a net decimal exponent E = exponent - fraction digits with
// |E| <= 44.  Its value is d = (double)m, times or over 10^min(|E|, 22), and when |E| > 22 times or over 10^(|E| - 22):
// at most three IEEE roundings, |d - x| <= 3 ulp(d).  An f32 rounding tie in the normal range is an f64 whose low 29
// significand bits are 0x10000000; when d's differ from that pattern by more than 4, x, RN64(x) and d lie on one side of
// every tie and (float)d is strtof's value and (float)strtod's.  Anything else is declined with a reason and parsed by
// the host.  Build with no fast-math and no contraction.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define FR_TEXT_HD __host__ __device__
#else
#define FR_TEXT_HD
#endif

namespace frtext {

// why a line goes back to the host parser; of several on one line the smallest code is the one counted
enum Reason : uint32_t { R_NONE = 0, R_TOO_LONG = 1, R_GRAMMAR = 2, R_NUMBER = 3, R_UNSORTED = 4, R_RANGE = 5, R_NEAR_TIE = 6, R_COUNT = 7 };
inline const char* reason_name(uint32_t r) {
    static const char* const names[R_COUNT] = {"none", "too_long", "grammar", "number", "unsorted", "range", "near_tie"};
    return r < R_COUNT ? names[r] : "?";
}

constexpr int MAX_SIG_DIGITS = 19, MAX_NET_EXP = 44, MAX_EXP_DIGITS = 4, MAX_FID_DIGITS = 9;

// C-locale isspace
FR_TEXT_HD inline bool is_space(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// the exact f64 powers 10^0 .. 10^22, as bit patterns (a table the host and the device read alike)
FR_TEXT_HD inline double pow10_exact(int k) {
    switch (k) {
        case 0: return 1e0;
        case 1: return 1e1;
        case 2: return 1e2;
        case 3: return 1e3;
        case 4: return 1e4;
        case 5: return 1e5;
        case 6: return 1e6;
        case 7: return 1e7;
        case 8: return 1e8;
        case 9: return 1e9;
        case 10: return 1e10;
        case 11: return 1e11;
        case 12: return 1e12;
        case 13: return 1e13;
        case 14: return 1e14;
        case 15: return 1e15;
        case 16: return 1e16;
        case 17: return 1e17;
        case 18: return 1e18;
        case 19: return 1e19;
        case 20: return 1e20;
        case 21: return 1e21;
        default: return 1e22;
    }
}

// s[0 .. len): one token.  R_NONE: *value is the f64 d of the rule and (float)d the correctly rounded f32.
FR_TEXT_HD inline uint32_t fast_number(const unsigned char* s, uint32_t len, double* value) {
    uint32_t i = 0;
    bool neg = false;
    if (i < len && (s[i] == '-' || s[i] == '+')) neg = s[i] == '-', i++;
    uint64_t m = 0;
    int sig = 0, frac = 0, digits = 0;
    bool dot = false;
    for (; i < len; i++) {
        const unsigned char c = s[i];
        if (c == '.') {
            if (dot) return R_NUMBER;
            dot = true;
            continue;
        }
        if (c < '0' || c > '9') break;
        digits++;
        if (dot) frac++;
        if (sig > 0 || c != '0') {
            if (++sig > MAX_SIG_DIGITS) return R_NUMBER;
            m = m * 10u + (uint64_t)(c - '0');
        }
    }
    if (digits == 0) return R_NUMBER;
    int ex = 0;
    if (i < len) {
        if (s[i] != 'e' && s[i] != 'E') return R_NUMBER;
        i++;
        bool eneg = false;
        if (i < len && (s[i] == '-' || s[i] == '+')) eneg = s[i] == '-', i++;
        const uint32_t e0 = i;
        for (; i < len && s[i] >= '0' && s[i] <= '9'; i++) ex = ex * 10 + (int)(s[i] - '0');
        if (i == e0 || i - e0 > (uint32_t)MAX_EXP_DIGITS || i != len) return R_NUMBER;
        if (eneg) ex = -ex;
    }
    const int E = ex - frac;
    const int a = E < 0 ? -E : E;
    if (a > MAX_NET_EXP) return R_NUMBER;
    double d = (double)m;
    const double p1 = pow10_exact(a < 22 ? a : 22);
    d = E < 0 ? d / p1 : d * p1;
    if (a > 22) {
        const double p2 = pow10_exact(a - 22);
        d = E < 0 ? d / p2 : d * p2;
    }
    if (m != 0 && (d < 1.1754943508222875e-38 /* 2^-126 */ || d > 3.4e38)) return R_RANGE;
    uint64_t bits;
    memcpy(&bits, &d, sizeof(bits));
    const int64_t low = (int64_t)(bits & 0x1FFFFFFFull) - 0x10000000ll;
    if (low >= -4 && low <= 4) return R_NEAR_TIE;
    *value = neg ? -d : d;
    return R_NONE;
}

// digits{1,9}: a feature id
FR_TEXT_HD inline bool fast_fid(const unsigned char* s, uint32_t len, uint32_t* fid) {
    if (len == 0 || len > (uint32_t)MAX_FID_DIGITS) return false;
    uint32_t v = 0;
    for (uint32_t i = 0; i < len; i++) {
        if (s[i] < '0' || s[i] > '9') return false;
        v = v * 10u + (uint32_t)(s[i] - '0');
    }
    *fid = v;
    return true;
}

}  // namespace frtext
