// Micro-benchmark: LambdaMART's GOSS select chain (fastrank_amd/csrc/kernels_goss.inc: six goss_hist_kernel / goss_pick_kernel
// pairs, no host synchronisation between them) against rocPRIM's radix_sort_keys of the same 64-bit keys, which is what the
// selection of the n-th largest |lambda| would otherwise cost.  3.8 M keys (the 30K shape's instance list), |lambda| drawn as
// |normal| x exp(normal), a third of them exact zeros.  Prints one JSON line; checks tau against the sorted keys.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/ubench/goss_select.hip -o tools/ubench/goss_select
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

// (kernels_goss.inc borrows the listwise objective's counter-based stream; the flag stage is not timed here)
__device__ __forceinline__ double xe_gamma(uint64_t key, uint32_t id) {
    uint64_t z = key + 0x9E3779B97F4A7C15ull * ((uint64_t)id + 1ull);
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-53;
}
#include "../../fastrank_amd/csrc/kernels_goss.inc"

#define CK(x)                                                                       \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                     \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));            \
            return 1;                                                               \
        }                                                                           \
    } while (0)

static float median(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? (uint32_t)std::atol(argv[1]) : 3800000u;
    const double rate = argc > 2 ? std::atof(argv[2]) : 0.2;
    const int reps = 30;
    const uint32_t n_top = std::max<uint32_t>(1, (uint32_t)((double)n * rate));
    std::mt19937_64 gen(1);
    std::normal_distribution<double> normal;
    std::vector<double> lam(n);
    std::vector<uint32_t> pos(n);
    for (uint32_t i = 0; i < n; i++) {
        lam[i] = gen() % 3 == 0 ? 0.0 : normal(gen) * std::exp(normal(gen));
        pos[i] = i;
    }
    double* d_lam;
    uint32_t *d_pos, *d_hist;
    unsigned long long *d_keys, *d_sorted;
    GossStateDev* d_st;
    CK(hipMalloc(&d_lam, n * sizeof(double)));
    CK(hipMalloc(&d_pos, n * sizeof(uint32_t)));
    CK(hipMalloc(&d_keys, n * sizeof(unsigned long long)));
    CK(hipMalloc(&d_sorted, n * sizeof(unsigned long long)));
    CK(hipMalloc(&d_hist, GOSS_PASSES * GOSS_BINS * sizeof(uint32_t)));
    CK(hipMalloc(&d_st, sizeof(GossStateDev)));
    CK(hipMemcpy(d_lam, lam.data(), n * sizeof(double), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_pos, pos.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    size_t temp_bytes = 0;
    CK(rocprim::radix_sort_keys(nullptr, temp_bytes, d_keys, d_sorted, n, 0u, 64u, 0));
    void* d_temp;
    CK(hipMalloc(&d_temp, std::max<size_t>(temp_bytes, 16)));
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    std::vector<float> t_select, t_sort;
    const unsigned g = (n + GOSS_SHARE - 1) / GOSS_SHARE;
    for (int r = 0; r < reps + 3; r++) {  // (three untimed rounds first)
        CK(hipEventRecord(a, 0));
        CK(hipMemsetAsync(d_hist, 0, GOSS_PASSES * GOSS_BINS * sizeof(uint32_t), 0));
        for (uint32_t pass = 0; pass < GOSS_PASSES; pass++) {
            if (pass == 0) goss_hist_kernel<true><<<g, 256, 0, 0>>>(d_lam, d_pos, nullptr, n, pass, d_st, d_keys, d_hist);
            else goss_hist_kernel<false><<<g, 256, 0, 0>>>(d_lam, d_pos, nullptr, n, pass, d_st, d_keys, d_hist);
            goss_pick_kernel<<<1, 64, 0, 0>>>(d_hist, pass, n_top, d_st);
        }
        CK(hipEventRecord(b, 0));
        CK(hipEventSynchronize(b));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, a, b));
        if (r >= 3) t_select.push_back(ms);
        CK(hipEventRecord(a, 0));
        size_t tb = temp_bytes;
        CK(rocprim::radix_sort_keys(d_temp, tb, d_keys, d_sorted, n, 0u, 64u, 0));
        CK(hipEventRecord(b, 0));
        CK(hipEventSynchronize(b));
        CK(hipEventElapsedTime(&ms, a, b));
        if (r >= 3) t_sort.push_back(ms);
    }
    CK(hipGetLastError());
    GossStateDev st{};
    unsigned long long want = 0;
    CK(hipMemcpy(&st, d_st, sizeof(st), hipMemcpyDeviceToHost));
    CK(hipMemcpy(&want, d_sorted + (n - n_top), sizeof(want), hipMemcpyDeviceToHost));
    std::printf("{\"n\": %u, \"n_top\": %u, \"reps\": %d, \"select_chain_ms_median\": %.4f, \"select_chain_ms_min\": %.4f, "
                "\"radix_sort_keys_ms_median\": %.4f, \"radix_sort_keys_ms_min\": %.4f, \"tau\": \"%016llx\", \"tau_matches_sort\": %s}\n",
                n, n_top, reps, median(t_select), *std::min_element(t_select.begin(), t_select.end()), median(t_sort),
                *std::min_element(t_sort.begin(), t_sort.end()), st.prefix, st.prefix == want ? "true" : "false");
    return st.prefix == want ? 0 : 2;
}
