// csrc/lambdamart_quant.hpp run on its own under -fsanitize=address,undefined (tests/test_lambdamart_quant_host.py builds and
// runs this): the key stream, the shifts at the ends of the list lengths, the quantised values at both extremes of Q and W for
// every key tried, and the packed histogram cell filled with HIST_CHUNK entries of every extreme pair, for 2 and 8 bits, and
// with random mixtures -- each decoded and held to sums kept in plain 64-bit integers ("Quantised
// gradients").
#include "lambdamart_quant.hpp"

#include "lambdamart_goss.hpp"

#include <cstdio>
#include <cstdlib>

using namespace fr;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

int main() {
    const uint64_t seeds[] = {0, 1, 0x8000000000000000ull, 0xFFFFFFFFFFFFFFFFull, QUANT_STREAM};
    for (uint64_t seed : seeds) {
        QuantKeys keys(seed);
        Rand64 same(seed ^ QUANT_STREAM), master(seed), goss(seed ^ GOSS_STREAM);
        for (uint32_t t = 0; t < 40; t++) {
            const uint64_t k = keys.next();
            CHECK(k == same.rand_u64());
            if (t < 6) CHECK(QuantKeys::of_tree(seed, t) == k);
        }
        if (seed != QUANT_STREAM) CHECK(QuantKeys::of_tree(seed, 0) != master.rand_u64());
        CHECK(QuantKeys::of_tree(seed, 0) != goss.rand_u64());
    }
    // the shifts: c = the bit length of n; at most 59, and at least 22 for every list the grower takes (fewer than 2^31 entries)
    const uint32_t lens[] = {1u, 2u, 3u, 4u, 255u, 256u, 8191u, 8192u, 3800000u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    for (uint32_t n : lens) {
        uint32_t c = 0;
        while (c < 32 && (n >> c) != 0) c++;
        CHECK(quant_bit_length(n) == c);
        for (uint32_t b = QUANT_MIN_BITS; b <= QUANT_MAX_BITS; b++) {
            const QuantShifts s = quant_shifts(n, b);
            CHECK(s.d == 62 - (int)c - (int)b && s.d_w == s.d - 1 && s.d_w >= 21 && s.d <= 59);
            if (n <= 0x7FFFFFFFu) CHECK(s.d_w >= 22);
            // the extremes of the fixed-point step, for every key and id tried: q = -+2^(b-1), w = 2^b and 0
            const int64_t top = (int64_t)1 << (61 - (int)c);
            const uint32_t ids[] = {0u, 1u, 63u, 0x7FFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu};
            for (uint64_t key : seeds)
                for (uint32_t id : ids) {
                    CHECK(quant_offset(key, id, 1u, s.d) < (1ull << s.d) && quant_offset(key, id, 2u, s.d_w) < (1ull << s.d_w));
                    CHECK(quant_q(top, key, id, s.d) == (int32_t)(1u << (b - 1)) && quant_q(-top, key, id, s.d) == -(int32_t)(1u << (b - 1)));
                    CHECK(quant_w(top, key, id, s.d_w) == (1u << b) && quant_w(0, key, id, s.d_w) == 0u);
                    CHECK(quant_q(0, key, id, s.d) == 0);
                    // a multiple of 2^d comes back as itself, one below it as itself or one less
                    const int64_t three = (int64_t)3 << s.d;
                    if (three <= top) CHECK(quant_q(-three, key, id, s.d) == -3 && quant_q(three, key, id, s.d) == 3);
                    const int32_t near = quant_q(-((int64_t)1 << s.d) - 1, key, id, s.d);
                    CHECK(near == -1 || near == -2);
                }
        }
    }
    // an entry's pair survives its u32
    for (int32_t q = -128; q <= 128; q++)
        for (uint32_t w = 0; w <= 256; w += (w < 8 || w >= 250) ? 1 : 37) {
            const uint32_t p = quant_pack(q, w);
            CHECK(quant_unpack_q(p) == q && quant_unpack_w(p) == w);
        }
    // a cell filled with QUANT_CHUNK entries of each extreme pair decodes to the three sums, for 2 and 8 bits
    for (uint32_t b : {QUANT_MIN_BITS, QUANT_MAX_BITS}) {
        const int32_t qm = (int32_t)(1u << (b - 1));
        const uint32_t wm = 1u << b;
        for (int32_t q : {-qm, 0, qm})
            for (uint32_t w : {0u, wm}) {
                uint64_t cell = 0;
                for (uint32_t i = 0; i < QUANT_CHUNK; i++) {
                    cell += quant_cell_add(quant_pack(q, w));
                    if (i == 0 || i + 1 == QUANT_CHUNK) {
                        CHECK(quant_cell_count(cell) == i + 1 && quant_cell_w(cell) == (uint64_t)w * (i + 1) && quant_cell_q(cell) == (int64_t)q * (int64_t)(i + 1));
                    }
                }
                CHECK(cell != 0);
            }
    }
    // random mixtures, the sums kept beside the cell
    uint64_t state = 12345;
    for (int round = 0; round < 50; round++) {
        const uint32_t b = QUANT_MIN_BITS + (uint32_t)(round % 7), count = round % 5 == 0 ? QUANT_CHUNK : 1 + (uint32_t)(quant_mix(state++) % QUANT_CHUNK);
        const int32_t qm = (int32_t)(1u << (b - 1));
        uint64_t cell = 0, sw = 0;
        int64_t sq = 0;
        for (uint32_t i = 0; i < count; i++) {
            const uint64_t r = quant_mix(state++);
            const int32_t q = (int32_t)(r % (uint64_t)(2 * qm + 1)) - qm;
            const uint32_t w = (uint32_t)((r >> 32) % ((1u << b) + 1u));
            cell += quant_cell_add(quant_pack(q, w));
            sq += q, sw += w;
        }
        CHECK(quant_cell_count(cell) == count && quant_cell_w(cell) == sw && quant_cell_q(cell) == sq);
    }
    CHECK(quant_bits_ok(0) && !quant_bits_ok(1) && quant_bits_ok(2) && quant_bits_ok(8) && !quant_bits_ok(9) && !quant_bits_ok(0xFFFFFFFFu));
    std::printf("lambdamart_quant ok\n");
    return 0;
}
