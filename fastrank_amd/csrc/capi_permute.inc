// ---------------------------------------------------------------------------------------------
// Permutation importance (DESIGN.md section 16; csrc/permute_host.hpp, kernels_permute.inc)
// ---------------------------------------------------------------------------------------------
extern "C" {

namespace {

// I (the view's instance ids ascending) and, for scope "query", each one's query
void permute_view_lists(const fr::DatasetView& view, bool per_query, std::vector<uint32_t>* ids, std::vector<uint32_t>* query_of) {
    *ids = view.instances;
    std::sort(ids->begin(), ids->end());
    query_of->clear();
    if (per_query)
        for (uint32_t id : *ids) query_of->push_back(view.core->qix[id]);
}

struct PermuteEnd {
    frdev::DeviceDataset& dev;
    ~PermuteEnd() { dev.permute_end(); }
};

}  // namespace

const void* fr_permutation_importance(const CModel* model, const CDataset* dataset, const CQRel* qrel, const void* evaluator_name, const void* options_json,
                                      double* out_values, size_t out_len, double* out_per_query) {
    return json_call([&]() {
        using clk = std::chrono::steady_clock;
        auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
        const CModel& cm = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        const std::string name = accept_str("evaluator_name", evaluator_name);
        const fr::PermuteOptions op = fr::permute_options_from_json(parse_json_or_fail(accept_str("options_json", options_json)));
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        const fr::Model& m = cm.actual;
        // every refusal that needs no device
        const fr::PermuteShape shape = fr::permute_model_shape(m);
        const std::vector<uint32_t> feats = fr::permute_features(op, view.features);
        if (view.instances.empty()) fr::fail_str("invalid value: permutation importance needs at least one document");
        const size_t F = feats.size(), R = op.repeats;
        if (F * R > 0 && !out_values) fr::fail_str("NULL pointer: out_values");
        if (out_len < F * R) fr::fail_str("fr_permutation_importance: output buffer too small");
        fr::Evaluator ev = fr::make_evaluator(view, name, qrel ? &qrel->actual : nullptr);

        frdev::DeviceDataset& dev = view.device();
        const size_t Q = dev.nq(), d = dev.d();
        std::string err;
        frdev::PermuteStats stats;
        // the baseline: fr_evaluate_dense's path on the view itself
        const auto t_base = clk::now();
        double baseline = 0.0;
        std::vector<double> base_pq(Q);
        fr::score_model(view, m);
        evaluate_scores(dev, ev, 1);
        if (!dev.reduce_means(1, &baseline, &err) || !dev.download_per_query(1, base_pq.data(), &err)) fr::fail_str(err);
        const double baseline_ms = ms_since(t_base);

        // which features are launched for: a feature past the matrix reads 0.0 whatever the rows are
        const std::vector<double>& colmax = dev.column_absmax();
        std::vector<std::pair<uint32_t, size_t>> run;  // (feature, its index in feats), ascending by feature
        std::vector<uint32_t> skipped;
        for (size_t fi = 0; fi < F; fi++) {
            if (feats[fi] < d && (!op.skip_unused || fr::permute_feature_used(m, feats[fi], colmax)))
                run.emplace_back(feats[fi], fi);
            else
                skipped.push_back(feats[fi]);
        }
        std::sort(run.begin(), run.end());
        for (size_t i = 0; i < F * R; i++) out_values[i] = baseline;
        if (out_per_query) {
            for (size_t b = 0; b <= F * R; b++) std::memcpy(out_per_query + b * Q, base_pq.data(), Q * sizeof(double));
        }

        size_t chunks = 0, max_slots_used = 0;
        double metric_ms = 0.0, sources_ms = 0.0;
        if (!run.empty()) {
            // one permutation per (seed, r), as positions
            const auto t_src = clk::now();
            std::vector<uint32_t> ids, query_of;
            permute_view_lists(view, op.per_query, &ids, &query_of);
            size_t np = 0;
            const uint32_t* instance_at = dev.position_instances(&np);
            const std::vector<uint32_t> pos = fr::permute_position_table(instance_at, np, ids.data(), ids.size());
            std::vector<uint32_t> src_pos(R * np);
            {  // the repeats are independent: one host sort each, side by side
                const size_t nthreads = std::max<size_t>(1, std::min<size_t>({R, 16, (size_t)std::max(1u, std::thread::hardware_concurrency())}));
                auto work = [&](size_t tid) {
                    std::vector<uint32_t> src_index(ids.size());
                    for (size_t r = tid; r < R; r += nthreads) {
                        fr::permute_sources(op.seed, (uint32_t)r, op.per_query ? query_of.data() : nullptr, ids.size(), src_index.data());
                        fr::permute_positions(pos.data(), src_index.data(), ids.size(), np, src_pos.data() + r * np);
                    }
                };
                std::vector<std::thread> pool;
                for (size_t tid = 1; tid < nthreads; tid++) pool.emplace_back(work, tid);
                work(0);
                for (auto& th : pool) th.join();
            }
            sources_ms = ms_since(t_src);
            PermuteEnd guard{dev};
            if (!dev.permute_begin(src_pos.data(), (uint32_t)R, &stats, &err)) fr::fail_str(err);
            const fr::PermuteModel pm = fr::permute_model(m, shape, d);
            const bool ensemble = shape == fr::PermuteShape::ENSEMBLE_LINEAR;
            const size_t C = dev.permute_chunk_features(run.size(), (uint32_t)R, (size_t)op.max_slots, ensemble ? 2 : 1);
            std::vector<uint32_t> chunk_feats;
            std::vector<double> vals, pq;
            for (size_t c0 = 0; c0 < run.size(); c0 += C) {
                const size_t nf = std::min(C, run.size() - c0), B = nf * R;
                chunk_feats.resize(nf);
                for (size_t k = 0; k < nf; k++) chunk_feats[k] = run[c0 + k].first;
                if (!dev.permute_score(chunk_feats.data(), nf, pm.members, ensemble, &stats, &err)) fr::fail_str(err);
                const auto t_metric = clk::now();
                evaluate_scores(dev, ev, B);
                vals.resize(B);
                if (!dev.reduce_means(B, vals.data(), &err)) fr::fail_str(err);
                metric_ms += ms_since(t_metric);
                if (out_per_query) {
                    pq.resize(Q * B);
                    if (!dev.download_per_query(B, pq.data(), &err)) fr::fail_str(err);
                }
                for (size_t k = 0; k < nf; k++) {
                    const size_t fi = run[c0 + k].second;
                    for (size_t r = 0; r < R; r++) {
                        out_values[fi * R + r] = vals[k * R + r];
                        if (out_per_query)
                            for (size_t q = 0; q < Q; q++) out_per_query[(fi * R + r) * Q + q] = pq[q * B + k * R + r];
                    }
                }
                chunks++;
                max_slots_used = std::max(max_slots_used, B);
            }
        }

        Value o = Value::object(), jf = Value::array(), jn = Value::array(), ji = Value::array(), js = Value::array(), jk = Value::array();
        for (size_t fi = 0; fi < F; fi++) {
            const fr::PermuteScore s = fr::permute_report(baseline, out_values + fi * R, R);
            jf.push(Value::uint(feats[fi])), jn.push(Value::string(view.core->feature_name(feats[fi])));
            ji.push(Value::number(s.importance)), js.push(Value::number(s.std));
        }
        for (uint32_t f : skipped) jk.push(Value::uint(f));
        o.set("features", jf), o.set("names", jn), o.set("baseline", Value::number(baseline)), o.set("importance", ji), o.set("std", js);
        o.set("skipped", jk), o.set("repeats", Value::uint(R)), o.set("seed", Value::uint(op.seed));
        o.set("scope", Value::string(op.per_query ? "query" : "dataset")), o.set("evaluator", Value::string(ev.name)), o.set("queries", Value::uint(Q));
        Value st = Value::object(), jl = Value::object();
        st.set("gather", Value::string(run.empty() ? "none" : (stats.gather_xcol ? "xcol" : "tiles")));
        st.set("rows", Value::string(stats.rows_in_lds ? "lds" : "global"));
        st.set("chunks", Value::uint(chunks)), st.set("slots", Value::uint(max_slots_used));
        st.set("score_ms", Value::number(stats.score_ms)), st.set("metric_ms", Value::number(metric_ms)), st.set("upload_ms", Value::number(stats.upload_ms));
        st.set("baseline_ms", Value::number(baseline_ms)), st.set("sources_ms", Value::number(sources_ms));
        jl.set("linear", Value::uint(stats.launches_linear)), jl.set("single", Value::uint(stats.launches_single));
        jl.set("trees", Value::uint(stats.launches_trees)), jl.set("axpy", Value::uint(stats.launches_axpy));
        st.set("launches", jl);
        o.set("stats", st);
        return frjson::dump(o);
    });
}

}  // extern "C"
