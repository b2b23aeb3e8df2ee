// Interface between the resampling report (resample_host.hpp, compiled into capi.o) and the resampling kernels
// (kernels_resample.inc + resample.inc, compiled into device.o).  DESIGN.md section 15.  No HIP.
//
// Input: V[Q][M] row-major f64, row q = one query's value under each of M systems; 1 <= M <= 8, 1 <= Q < 2^32,
// 1 <= T <= 2^20 trials, a u64 seed.  All integer arithmetic is mod 2^64:
//   G = 0x9E3779B97F4A7C15, mix = the splitmix64 finaliser, K_B = mix(seed + 1 G), K_P = mix(seed + 2 G)
//   SUM(x_0 .. x_{Q-1})   segments of SEG = 256 consecutive terms, each added one after the other from +0.0; the partials added
//                         one after the other from +0.0 (the shape of the mean over queries); no FMA
//   bootstrap             i(t,k) = ((mix(K_B + G (t Q + k + 1)) >> 32) Q) >> 32;  boot[t][c] = SUM_k V[i(t,k)][c] / Q
//   permutation           r = ((mix(K_P + G (t Q + q + 1)) >> 32) M!) >> 32; p = identity; for i = M-1 .. 1: j = r mod (i+1),
//                         r = r div (i+1), swap p[i], p[j];  perm[t][c] = SUM_q V[q][p[c]] / Q
// A trial's stream depends on (seed, t, Q) alone, never on T.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace frresample {

constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr uint32_t SEG = 256;
constexpr uint32_t MAX_SYSTEMS = 8;
constexpr uint32_t MAX_TRIALS = 1u << 20;
constexpr uint32_t LDS_BLOCK = 512;           // lanes of a workgroup of the bootstrap kernel's LDS form
constexpr size_t LDS_BYTES = 128u * 1024u;    // the largest table that form stages: a CU's 160 KiB less room for the rest

inline uint64_t mix(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
inline uint64_t boot_key(uint64_t seed) { return mix(seed + 1ull * GOLDEN); }
inline uint64_t perm_key(uint64_t seed) { return mix(seed + 2ull * GOLDEN); }

}  // namespace frresample

namespace frdev {

struct ResampleTimes {
    bool lds = false;  // the bootstrap kernel gathered from LDS
    double boot_ms = 0, perm_ms = 0, upload_ms = 0, download_ms = 0;
};

// Uploads V[Q][M] to the current device, runs the bootstrap kernel when boot != nullptr and the permutation kernel when perm
// != nullptr, and downloads their T x M results.  The caller has checked the limits above.  false: *err holds the reason (no
// device: the `no MI355X/HIP device available...` text).
bool resample_run(const double* V, size_t Q, uint32_t M, uint32_t T, uint64_t seed, double* boot, double* perm, ResampleTimes* times, std::string* err);

}  // namespace frdev
