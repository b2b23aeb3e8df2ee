// Part of device.hip (single translation unit; see that file's header).  The launcher of kernels_resample.inc (DESIGN.md
// section 15): one upload of the table, at most two kernels, two downloads, every stage between two events of one stream.

namespace {

struct ResampleStream {
    hipStream_t st = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~ResampleStream() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
};

template <int M>
bool resample_launch(const double* dV, uint32_t Q, uint32_t T, uint64_t seed, double* dboot, double* dperm, bool lds, ResampleStream& rs,
                     std::string* err) {
    FR_HIP(hipEventRecord(rs.ev[1], rs.st));
    if (dboot) {
        ProfScope ps("resample_boot_kernel", rs.st);
        const uint64_t key = frresample::boot_key(seed);
        if (lds) {
            const size_t bytes = (size_t)Q * M * sizeof(double);
            FR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&resample_boot_kernel<M, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)frresample::LDS_BYTES));
            resample_boot_kernel<M, true><<<(T + frresample::LDS_BLOCK - 1) / frresample::LDS_BLOCK, frresample::LDS_BLOCK, bytes, rs.st>>>(dV, Q, T, key, dboot);
        } else {
            resample_boot_kernel<M, false><<<(T + 63u) / 64u, 64, 0, rs.st>>>(dV, Q, T, key, dboot);
        }
        FR_HIP(hipGetLastError());
    }
    FR_HIP(hipEventRecord(rs.ev[2], rs.st));
    if (dperm) {
        ProfScope ps("resample_perm_kernel", rs.st);
        resample_perm_kernel<M><<<(T + 63u) / 64u, 64, 0, rs.st>>>(dV, Q, T, frresample::perm_key(seed), dperm);
        FR_HIP(hipGetLastError());
    }
    FR_HIP(hipEventRecord(rs.ev[3], rs.st));
    return true;
}

}  // namespace

bool resample_run(const double* V, size_t Q, uint32_t M, uint32_t T, uint64_t seed, double* boot, double* perm, ResampleTimes* times, std::string* err) {
    std::string e2;
    if (device_count(&e2) <= 0) {
        if (err) *err = "no MI355X/HIP device available for the fastrank_amd compute path (" + (e2.empty() ? std::string("device count is 0") : e2) + ")";
        return false;
    }
    if (Q == 0 || Q > 0xFFFFFFFFull || M == 0 || M > frresample::MAX_SYSTEMS || T == 0 || T > frresample::MAX_TRIALS) {
        if (err) *err = "resample_run: a size outside the kernels' limits";
        return false;
    }
    const size_t cells = Q * M, out_cells = (size_t)T * M;
    // the LDS form: the whole table beside the lanes of one workgroup (FR_RESAMPLE_BOOT=global: the other bit-exact path)
    const char* force = path_env("FR_RESAMPLE_BOOT");
    const bool lds = cells * sizeof(double) <= frresample::LDS_BYTES && !(force && std::strcmp(force, "global") == 0);
    DevBuf<double> dV, dboot, dperm;
    ResampleStream rs;
    FR_HIP(hipStreamCreateWithFlags(&rs.st, hipStreamNonBlocking));
    for (hipEvent_t& e : rs.ev) FR_HIP(hipEventCreate(&e));
    if (!dV.ensure(cells, err) || (boot && !dboot.ensure(out_cells, err)) || (perm && !dperm.ensure(out_cells, err))) return false;
    FR_HIP(hipEventRecord(rs.ev[0], rs.st));
    FR_HIP(hipMemcpyAsync(dV.p, V, cells * sizeof(double), hipMemcpyHostToDevice, rs.st));
    bool ok = false;
    switch (M) {
        case 1: ok = resample_launch<1>(dV.p, (uint32_t)Q, T, seed, dboot.p, dperm.p, lds, rs, err); break;
        case 2: ok = resample_launch<2>(dV.p, (uint32_t)Q, T, seed, dboot.p, dperm.p, lds, rs, err); break;
        case 3: ok = resample_launch<3>(dV.p, (uint32_t)Q, T, seed, dboot.p, dperm.p, lds, rs, err); break;
        case 4: ok = resample_launch<4>(dV.p, (uint32_t)Q, T, seed, dboot.p, dperm.p, lds, rs, err); break;
        case 5: ok = resample_launch<5>(dV.p, (uint32_t)Q, T, seed, dboot.p, dperm.p, lds, rs, err); break;
        case 6: ok = resample_launch<6>(dV.p, (uint32_t)Q, T, seed, dboot.p, dperm.p, lds, rs, err); break;
        case 7: ok = resample_launch<7>(dV.p, (uint32_t)Q, T, seed, dboot.p, dperm.p, lds, rs, err); break;
        default: ok = resample_launch<8>(dV.p, (uint32_t)Q, T, seed, dboot.p, dperm.p, lds, rs, err); break;
    }
    if (!ok) {
        (void)hipStreamSynchronize(rs.st);
        return false;
    }
    if (boot) FR_HIP(hipMemcpyAsync(boot, dboot.p, out_cells * sizeof(double), hipMemcpyDeviceToHost, rs.st));
    if (perm) FR_HIP(hipMemcpyAsync(perm, dperm.p, out_cells * sizeof(double), hipMemcpyDeviceToHost, rs.st));
    FR_HIP(hipEventRecord(rs.ev[4], rs.st));
    FR_HIP(hipStreamSynchronize(rs.st));
    if (times) {
        auto ms = [&](int a, int b) {
            float f = 0.0f;
            return hipEventElapsedTime(&f, rs.ev[a], rs.ev[b]) == hipSuccess ? (double)f : 0.0;
        };
        times->lds = lds && boot != nullptr;
        times->upload_ms = ms(0, 1), times->boot_ms = ms(1, 2), times->perm_ms = ms(2, 3), times->download_ms = ms(3, 4);
    }
    return true;
}
