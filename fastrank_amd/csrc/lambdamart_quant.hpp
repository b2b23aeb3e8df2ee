// LambdaMART's quantised gradients, host side ("Quantised gradients"; device side:
// kernels_histquant.inc).  Integer arithmetic only, shared with the device (the functions marked FR_QUANT_HD are the ones the
// kernels call), and the key stream.
//
//   key       tree t's key K_t is the t-th rand_u64() of Rand64(seed ^ QUANT_STREAM): a stream of its own, like the GOSS, DART
//             and listwise streams, so none of them moves.
//   shifts    after the fixed-point step |Q_i| <= 2^(61 - c) and 0 <= W_i <= 2^(61 - c), c = the bit length of the tree's list;
//             with b = grad_quant_bits, d = 62 - c - b and d_w = 61 - c - b (both >= 22, since c <= 32 and b <= 8).
//   offsets   r_i = mix(K_t + phi (2 id_i + 1)) >> (64 - d), r'_i = mix(K_t + phi (2 id_i + 2)) >> (64 - d_w), phi =
//             0x9E3779B97F4A7C15, mix = the splitmix64 finaliser, id = the document's original instance id.
//   values    q_i = (Q_i + r_i) >> d (arithmetic: floor), w_i = (W_i + r'_i) >> d_w: q in [-2^(b-1), 2^(b-1)], w in [0, 2^b],
//             and over a uniform r the mean of q_i is exactly Q_i / 2^d.
//   search    every sum the search reads is a sum of (1, q_i, w_i) under the exponents S - d and S_w - d_w.
//   leaves    are renewed from the full-precision sums of Q_i and W_i under (S, S_w).
//   packing   (q, w) of an entry as one u32 (q as i16 in the high half, w as u16 in the low half); an LDS histogram cell as
//             one u64 of three fields, bits 0..13 the count, 14..37 sum w, 38..63 sum q (two's complement), filled by adding
//             (q << 38) + (w << 14) + 1 in wrap-around arithmetic.  One workgroup adds at most QUANT_CHUNK entries to a cell:
//             the count is at most 2^13 (14 bits), sum w at most 2^13 2^8 = 2^21 (24 bits), |sum q| at most 2^13 2^7 = 2^20
//             (26 bits, signed); the fields below sum q hold a non-negative number, so the arithmetic shift by 38 is exact.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FR_QUANT_HD __host__ __device__ inline
#else
#define FR_QUANT_HD inline
#endif

namespace fr {

constexpr uint64_t QUANT_STREAM = 0x5155414E54475244ull;  // "QUANTGRD"
constexpr uint64_t QUANT_PHI = 0x9E3779B97F4A7C15ull;
constexpr uint32_t QUANT_MIN_BITS = 2, QUANT_MAX_BITS = 8;
constexpr uint32_t QUANT_CHUNK = 8192;  // entries one workgroup adds into its LDS histogram (= HIST_CHUNK, held there)
constexpr uint32_t QUANT_CNT_BITS = 14, QUANT_W_BITS = 24, QUANT_Q_BITS = 26;
constexpr uint32_t QUANT_W_SHIFT = QUANT_CNT_BITS, QUANT_Q_SHIFT = QUANT_CNT_BITS + QUANT_W_BITS;

static_assert(QUANT_CNT_BITS + QUANT_W_BITS + QUANT_Q_BITS == 64, "the three fields tile the word");
static_assert((uint64_t)QUANT_CHUNK < (1ull << QUANT_CNT_BITS), "a piece's count fits its field");
static_assert((uint64_t)QUANT_CHUNK * (1ull << QUANT_MAX_BITS) < (1ull << QUANT_W_BITS), "a piece's sum w fits its field");
static_assert((uint64_t)QUANT_CHUNK * (1ull << (QUANT_MAX_BITS - 1)) < (1ull << (QUANT_Q_BITS - 1)), "a piece's |sum q| fits its signed field");
static_assert((1u << (QUANT_MAX_BITS - 1)) <= 0x7FFFu && (1u << QUANT_MAX_BITS) <= 0xFFFFu, "q fits an i16 and w a u16");

inline bool quant_bits_ok(uint32_t bits) { return bits == 0 || (bits >= QUANT_MIN_BITS && bits <= QUANT_MAX_BITS); }

struct QuantShifts {
    int d, d_w;
};
// the bit length of n = ceil(log2(n + 1))
FR_QUANT_HD uint32_t quant_bit_length(uint32_t n) {
    uint32_t c = 0;
    for (; n != 0; n >>= 1) c++;
    return c;
}
FR_QUANT_HD QuantShifts quant_shifts(uint32_t n, uint32_t bits) {
    const int c = (int)quant_bit_length(n);
    return {62 - c - (int)bits, 61 - c - (int)bits};
}

FR_QUANT_HD uint64_t quant_mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// the random offset of document `id` under the tree key: which = 1 for q (shift = d), 2 for w (shift = d_w); 1 <= shift <= 63
FR_QUANT_HD uint64_t quant_offset(uint64_t key, uint32_t id, uint32_t which, int shift) {
    return quant_mix(key + QUANT_PHI * (2ull * (uint64_t)id + (uint64_t)which)) >> (64 - shift);
}
// floor((v + r) / 2^shift): the sum cannot overflow (|v| <= 2^61, r < 2^shift <= 2^60); a negative value's shift is the
// arithmetic one (C++20 defines it; every compiler this builds with does so before)
FR_QUANT_HD int64_t quant_round(int64_t v, uint64_t r, int shift) { return (v + (int64_t)r) >> shift; }
FR_QUANT_HD int32_t quant_q(int64_t Q, uint64_t key, uint32_t id, int d) { return (int32_t)quant_round(Q, quant_offset(key, id, 1u, d), d); }
FR_QUANT_HD uint32_t quant_w(int64_t W, uint64_t key, uint32_t id, int d_w) { return (uint32_t)quant_round(W, quant_offset(key, id, 2u, d_w), d_w); }

// an entry's pair as one u32
FR_QUANT_HD uint32_t quant_pack(int32_t q, uint32_t w) { return ((uint32_t)(uint16_t)(int16_t)q << 16) | (w & 0xFFFFu); }
FR_QUANT_HD int32_t quant_unpack_q(uint32_t p) { return (int32_t)(int16_t)(uint16_t)(p >> 16); }
FR_QUANT_HD uint32_t quant_unpack_w(uint32_t p) { return p & 0xFFFFu; }

// what an entry adds to its cell, and a cell's three sums back
FR_QUANT_HD uint64_t quant_cell_add(uint32_t packed) {
    return ((uint64_t)(int64_t)quant_unpack_q(packed) << QUANT_Q_SHIFT) + ((uint64_t)quant_unpack_w(packed) << QUANT_W_SHIFT) + 1ull;
}
FR_QUANT_HD uint32_t quant_cell_count(uint64_t v) { return (uint32_t)(v & ((1ull << QUANT_CNT_BITS) - 1ull)); }
FR_QUANT_HD uint64_t quant_cell_w(uint64_t v) { return (v >> QUANT_W_SHIFT) & ((1ull << QUANT_W_BITS) - 1ull); }
FR_QUANT_HD int64_t quant_cell_q(uint64_t v) { return (int64_t)v >> QUANT_Q_SHIFT; }

}  // namespace fr

#ifndef FR_QUANT_ARITHMETIC_ONLY  // (the device's translation unit takes the arithmetic alone)
#include "host.hpp"

namespace fr {

class QuantKeys {
  public:
    explicit QuantKeys(uint64_t seed) : gen_(seed ^ QUANT_STREAM) {}
    uint64_t next() { return gen_.rand_u64(); }  // K_0, K_1, ...: one per tree, in order
    // K_tree without keeping a stream
    static uint64_t of_tree(uint64_t seed, uint32_t tree) {
        QuantKeys k(seed);
        uint64_t out = 0;
        for (uint32_t t = 0; t <= tree; t++) out = k.next();
        return out;
    }

  private:
    Rand64 gen_;
};

}  // namespace fr
#endif
