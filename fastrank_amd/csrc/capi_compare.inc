// ---------------------------------------------------------------------------------------------
// Model comparison (DESIGN.md section 15; csrc/resample_host.hpp, kernels_resample.inc)
// ---------------------------------------------------------------------------------------------
extern "C" {

namespace {

// the checked table through both kernels (a null output skips its kernel), then the host's report with the call's stats
Value resample_table(const double* V, size_t Q, size_t M, const fr::ResampleOptions& op, double* boot, double* perm) {
    fr::resample_check(V, Q, M);
    frdev::ResampleTimes times;
    std::string err;
    const auto t0 = std::chrono::steady_clock::now();
    if (!frdev::resample_run(V, Q, (uint32_t)M, op.trials, op.seed, boot, perm, &times, &err)) fr::fail_str(err);
    const auto t1 = std::chrono::steady_clock::now();
    Value o = fr::resample_report(V, Q, M, op.trials, op.alpha, boot, perm);
    const auto t2 = std::chrono::steady_clock::now();
    o.set("trials", Value::uint(op.trials)), o.set("seed", Value::uint(op.seed)), o.set("alpha", Value::number(op.alpha));
    o.set("boot_path", Value::string(times.lds ? "lds" : "global"));
    o.set("boot_ms", Value::number(times.boot_ms)), o.set("perm_ms", Value::number(times.perm_ms));
    o.set("upload_ms", Value::number(times.upload_ms)), o.set("download_ms", Value::number(times.download_ms));
    o.set("device_call_ms", Value::number(std::chrono::duration<double, std::milli>(t1 - t0).count()));
    o.set("report_ms", Value::number(std::chrono::duration<double, std::milli>(t2 - t1).count()));
    return o;
}

}  // namespace

const void* fr_resample(const double* values, size_t nq, size_t ncols, const void* options_json, double* out_boot, double* out_perm) {
    return json_call([&]() {
        const fr::ResampleOptions op = fr::resample_options_from_json(parse_json_or_fail(accept_str("options_json", options_json)));
        return frjson::dump(resample_table(values, nq, ncols, op, out_boot, out_perm));
    });
}

const void* fr_compare_models(const CModel* const* models, size_t n_models, const CDataset* dataset, const CQRel* qrel, const void* evaluator_name,
                              const void* options_json) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        const std::string name = accept_str("evaluator_name", evaluator_name);
        const fr::ResampleOptions op = fr::resample_options_from_json(parse_json_or_fail(accept_str("options_json", options_json)));
        if (n_models < 1 || n_models > frresample::MAX_SYSTEMS)
            fr::fail_str("invalid value: a comparison takes between 1 and " + std::to_string(frresample::MAX_SYSTEMS) + " systems, not " + std::to_string(n_models));
        if (!models) fr::fail_str("NULL pointer: models");
        for (size_t c = 0; c < n_models; c++) require_model(models[c]);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        fr::Evaluator ev = fr::make_evaluator(view, name, qrel ? &qrel->actual : nullptr);
        if (view.instances.empty()) fr::fail_str("invalid value: a comparison needs at least one query");
        // every model through fr_evaluate_dense's path on the one view: the same queries in the same order for all
        frdev::DeviceDataset& dev = view.device();
        const size_t Q = dev.nq(), M = n_models;
        std::vector<double> V(Q * M), column(Q);
        std::string err;
        for (size_t c = 0; c < M; c++) {
            fr::score_model(view, models[c]->actual);
            evaluate_scores(dev, ev, 1);
            if (!dev.download_per_query(1, column.data(), &err)) fr::fail_str(err);
            for (size_t q = 0; q < Q; q++) V[q * M + c] = column[q];
        }
        std::vector<double> boot((size_t)op.trials * M), perm(M > 1 ? (size_t)op.trials * M : 0);  // (one system: nothing to permute)
        Value o = resample_table(V.data(), Q, M, op, boot.data(), M > 1 ? perm.data() : nullptr);
        o.set("queries", Value::uint(Q));
        return frjson::dump(o);
    });
}

}  // extern "C"
