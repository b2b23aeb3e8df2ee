// The reference's random numbers: its generator, its shuffle and its sampling count.  Plain C++ (no HIP, no environment);
// host.hpp includes it, so every trainer sees these names as before.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace fr {

// ---------------------------------------------------------------------------------------------
// Rand64 -- oorandom =11.1.0 (Cargo.toml:18-19), third-party, source absent from the reference
// tree: restated from the crate's published PCG algorithm.  Seed->trajectory parity with the
// Rust build is UNPINNED (DESIGN.md "Parity status").
// ---------------------------------------------------------------------------------------------
class Rand64 {
  public:
    explicit Rand64(uint64_t seed) {
        state_ = 0;
        inc_ = (default_inc() << 1) | 1;
        (void)rand_u64();
        state_ += (u128)seed;
        (void)rand_u64();
    }
    uint64_t rand_u64() {
        u128 old = state_;
        state_ = old * multiplier() + inc_;
        uint64_t xorshifted = (uint64_t)(((old >> 29) ^ old) >> 58);
        uint32_t rot = (uint32_t)(old >> 122);
        return (xorshifted >> rot) | (xorshifted << ((64 - rot) & 63));
    }
    double rand_float() {
        uint64_t u = rand_u64() >> (64 - 54);
        return (double)u * (1.0 / 18014398509481984.0);
    }
    uint64_t rand_range(uint64_t lo, uint64_t hi) {
        uint64_t s = hi - lo;
        u128 m = (u128)rand_u64() * (u128)s;
        uint64_t leftover = (uint64_t)m;
        if (leftover < s) {
            uint64_t threshold = (0 - s) % s;
            while (leftover < threshold) {
                m = (u128)rand_u64() * (u128)s;
                leftover = (uint64_t)m;
            }
        }
        return (uint64_t)(m >> 64) + lo;
    }

  private:
    typedef unsigned __int128 u128;
    static u128 multiplier() { return (((u128)2549297995355413924ULL) << 64) | (u128)4865540595714422341ULL; }
    static u128 default_inc() { return (((u128)0x2FE0E169FFBD06E3ULL) << 64) | (u128)0x5BC307BD4D2F814FULL; }
    u128 state_, inc_;
};

// src/randutil.rs:21-27
template <typename T>
inline void shuffle(std::vector<T>& v, Rand64& rand) {
    uint64_t n = v.size();
    for (uint64_t i = 0; i < n; i++) {
        uint64_t j = rand.rand_range(i, n);
        std::swap(v[i], v[j]);
    }
}

// sampling.rs:49-50: how many of `len` items a sampling rate keeps: max(1, (len as f64 * rate) as usize), at most len.
// Rust's cast saturates (NaN / negative -> 0); a C++ cast of such a value is undefined behaviour.  Shared by the
// random-forest trainer and LambdaMART's per-tree samples.
inline size_t sample_count(size_t len, double rate) {
    const double x = (double)len * rate;
    const size_t c = (x != x || x <= 0.0) ? 0 : (x >= (double)len ? len : (size_t)x);
    return std::min(len, std::max<size_t>(1, c));
}

}  // namespace fr
