// capi.cpp: the evaluation extensions (dense outputs instead of JSON), what a dataset handle can be asked, the loader that
// names its parser, and the process-wide calls.
namespace {

std::mutex g_load_mu;  // fr_last_load_stats
fr::LoadStats g_last_load;

}  // namespace

extern "C" {

const CResult* fr_load_ranksvm(const void* data_path, const void* feature_names_path, const void* parser) {
    return c_call<CDataset>([&]() {
        std::string path = accept_str("data_path", data_path);
        const std::string word = accept_str("parser", parser);
        std::map<uint32_t, std::string> names;
        bool has_names = false;
        if (feature_names_path) {
            names = fr::load_feature_names(accept_str("feature_names_path", feature_names_path));
            has_names = true;
        }
        fr::LoadStats st;
        CDataset* d = new_handle<CDataset>([&] { return fr::load_ranksvm_with(path, has_names ? &names : nullptr, word, &st); });
        std::lock_guard<std::mutex> lk(g_load_mu);
        g_last_load = st;
        return d;
    });
}

// what the last successful fr_load_ranksvm / load_ranksvm_format of this process did (include/fastrank.h)
const void* fr_last_load_stats(void) {
    return json_call([&]() {
        std::lock_guard<std::mutex> lk(g_load_mu);
        const fr::LoadStats& s = g_last_load;
        Value o = Value::object();
        o.set("parser", Value::string(s.parser));
        o.set("reason", Value::string(s.reason));
        o.set("bytes", Value::uint(s.bytes));
        o.set("lines", Value::uint(s.lines));
        o.set("host_lines", Value::uint(s.host_lines));
        Value r = Value::object();
        for (uint32_t k = 1; k < frtext::R_COUNT; k++) r.set(frtext::reason_name(k), Value::uint(s.reasons[k]));
        o.set("host_line_reasons", std::move(r));
        Value t = Value::object();
        t.set("read", Value::number(s.read)), t.set("upload", Value::number(s.dev.upload)), t.set("line_scan", Value::number(s.dev.line_scan));
        t.set("pass1", Value::number(s.dev.pass1)), t.set("pass2", Value::number(s.dev.pass2)), t.set("download", Value::number(s.dev.download));
        t.set("host_merge", Value::number(s.merge)), t.set("total", Value::number(s.total));
        o.set("seconds", std::move(t));
        o.set("scan_slice", Value::uint(frdev::TEXT_SCAN_SLICE));
        o.set("stage_limit", Value::uint(frdev::TEXT_STAGE_LIMIT));
        o.set("auto_threshold", Value::uint(fr::TEXT_DEVICE_THRESHOLD));
        return frjson::dump(o);
    });
}

int fr_device_count(void) { return frdev::device_count(nullptr); }

int fr_set_device(int ordinal) {
    std::string err;
    if (!frdev::set_device(ordinal, &err)) return 1;
    frdev::warm_device(ordinal);
    g_pinned_device = ordinal;  // train_model then stays on this device unless FR_DEVICES says otherwise
    return 0;
}

const char* fr_version(void) { return "fastrank_amd 0.1.0 (fastrank C ABI 0.9.0-dev / python 0.7.0)"; }

size_t fr_dataset_release_replicas(const CDataset* dataset) {
    if (!dataset || !dataset->view) return 0;
    std::lock_guard<std::mutex> lk(api_mu_of(*dataset));
    size_t n = 0;
    for (fr::DatasetView* v = dataset->view.get(); v; v = v->parent.get()) n += v->release_replicas();
    return n;
}

size_t fr_dataset_num_queries(const CDataset* dataset) {
    if (!dataset) return 0;
    // host_csr() validates the labels (a NaN label is an error): nothing may unwind through extern "C".
    // SIZE_MAX = "this dataset cannot be grouped"; the compute calls report the reason in their envelope.
    try {
        return dataset->view->host_csr().nq;
    } catch (...) {
        return SIZE_MAX;
    }
}

const void* fr_dataset_device_info(const CDataset* dataset) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        std::shared_ptr<frdev::DeviceDataset> devp = ds.view->device_ptr();
        frdev::DeviceDataset& dev = *devp;
        fr::DatasetView* owner = ds.view->matrix_owner(nullptr);
        const bool is_parents = owner != ds.view.get() && owner->device_ptr() == devp;  // a feature sample: the parent's object itself
        Value o = Value::object();
        o.set("hbm_bytes_owned", Value::uint(is_parents ? 0 : dev.hbm_bytes()));
        o.set("shares_parent_matrix", Value::boolean(is_parents || dev.shares_parent_matrix()));
        o.set("is_parent_device_dataset", Value::boolean(is_parents));
        o.set("queries", Value::uint(dev.nq()));
        o.set("instances", Value::uint(dev.n()));
        return frjson::dump(o);
    });
}

size_t fr_dataset_num_instances(const CDataset* dataset) {
    if (!dataset) return 0;
    return dataset->view->instances.size();
}

const void* fr_predict_scores_dense(const CModel* model, const CDataset* dataset, double* out, size_t out_len) {
    return status_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) return;
        frdev::DeviceDataset& dev = view.device();
        fr::score_model(view, m.actual);
        std::string err;
        if (!dev.download_scores(0, out, out_len, &err)) fr::fail_str(err);
    });
}

const void* fr_evaluate_dense(const CModel* model, const CDataset* dataset, const CQRel* qrel,
                              const void* evaluator_name, double* out_values, size_t out_len,
                              const void** out_qids_json) {
    return status_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::string name = accept_str("evaluator_name", evaluator_name);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        fr::Evaluator ev = fr::make_evaluator(view, name, qrel ? &qrel->actual : nullptr);
        frdev::DeviceDataset& dev = view.device();
        if (out_len < dev.nq()) fr::fail_str("fr_evaluate_dense: output buffer too small");
        fr::score_model(view, m.actual);
        evaluate_scores(dev, ev, 1);
        std::string err;
        if (!dev.download_per_query(1, out_values, &err)) fr::fail_str(err);
        if (out_qids_json) {
            Value a = Value::array();
            for (size_t q = 0; q < dev.nq(); q++) a.push(Value::string(view.core->qnames[view.csr_query[q]]));
            *out_qids_json = return_string(frjson::dump(a));
        }
    });
}

const void* fr_rank_order(const CModel* model, const CDataset* dataset, uint32_t* out_instance_ids, size_t n,
                          uint64_t* out_offsets, size_t nq_plus_1) {
    return status_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        frdev::DeviceDataset& dev = view.device();
        if (n < dev.n() || nq_plus_1 < dev.nq() + 1) fr::fail_str("fr_rank_order: output buffers too small");
        rank_view(view, m.actual);
        std::string err;
        if (!dev.download_rank(out_instance_ids, &err)) fr::fail_str(err);
        const frdev::HostCSR& csr = view.host_csr();
        for (size_t q = 0; q <= csr.nq; q++) out_offsets[q] = csr.qoff[q];
    });
}

const void* fr_evaluate_candidates(const CDataset* dataset, const CQRel* qrel, const void* evaluator_name,
                                   size_t n_groups, const uint32_t* features, const double* base_weights,
                                   const uint32_t* n_cand, const double* candidates, double* out_means,
                                   double* out_per_query) {
    return status_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        std::string name = accept_str("evaluator_name", evaluator_name);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        fr::Evaluator ev = fr::make_evaluator(view, name, qrel ? &qrel->actual : nullptr);
        frdev::DeviceDataset& dev = view.device();
        dev.set_sums_only(false);
        const size_t d = dev.d();
        std::string err;
        for (size_t g = 0; g < n_groups; g++)
            if (n_cand[g] == 0 || n_cand[g] > 64 || features[g] >= d)
                fr::fail_str("fr_evaluate_candidates: malformed group");
        if (dev.linesearch_path(ev.measure, ev.depth) != frdev::DeviceDataset::LS_NONE) {
            std::vector<frdev::LineGroup> groups(n_groups);
            for (size_t g = 0; g < n_groups; g++) {
                groups[g].feature = features[g];
                groups[g].weights.assign(base_weights + g * d, base_weights + (g + 1) * d);
                groups[g].candidates.assign(candidates + g * 64, candidates + g * 64 + n_cand[g]);
            }
            std::vector<double> means;
            if (!dev.linesearch(ev.measure, ev.depth, ev.norms.data(), groups, &means, nullptr, &err)) fr::fail_str(err);
            fr::check_flags(dev);
            std::copy(means.begin(), means.end(), out_means);
            // Slots no candidate fills hold 0, as on the generic path below: the device matrix is a grow-only work buffer, and
            // the kernels write only the candidates a group has, so those columns keep what an earlier, wider line search on
            // this dataset left there.
            for (size_t g = 0; g < n_groups; g++) std::fill(out_means + g * 64 + n_cand[g], out_means + (g + 1) * 64, 0.0);
            if (out_per_query) {
                std::vector<double> M;
                size_t ldm = 0;
                if (!dev.download_last_matrix(&M, &ldm, &err)) fr::fail_str(err);
                std::copy(M.begin(), M.end(), out_per_query);
                for (size_t q = 0; q < dev.nq() && ldm == n_groups * 64; q++)
                    for (size_t g = 0; g < n_groups; g++)
                        std::fill(out_per_query + q * ldm + g * 64 + n_cand[g], out_per_query + q * ldm + (g + 1) * 64, 0.0);
            }
        } else {
            std::vector<double> w;
            std::vector<size_t> slot;
            for (size_t g = 0; g < n_groups; g++)
                for (uint32_t c = 0; c < n_cand[g]; c++) {
                    size_t off = w.size();
                    w.insert(w.end(), base_weights + g * d, base_weights + (g + 1) * d);
                    w[off + features[g]] = candidates[g * 64 + c];
                    slot.push_back(g * 64 + c);
                }
            std::vector<double> means, pq;
            fr::evaluate_means_generic(view.device(), ev, w, slot.size(), means, out_per_query ? &pq : nullptr);
            for (size_t g = 0; g < n_groups * 64; g++) out_means[g] = 0.0;
            for (size_t k = 0; k < slot.size(); k++) out_means[slot[k]] = means[k];
            if (out_per_query) {  // [nq][n_groups * 64] as the fused paths give it; slots no candidate fills hold 0
                const size_t ld = n_groups * 64, B = slot.size();
                std::fill(out_per_query, out_per_query + dev.nq() * ld, 0.0);
                for (size_t q = 0; q < dev.nq(); q++)
                    for (size_t k = 0; k < B; k++) out_per_query[q * ld + slot[k]] = pq[q * B + k];
            }
        }
    });
}

void fr_profile_enable(int on) { frdev::profile_enable(on != 0); }
void fr_profile_reset(void) { frdev::profile_reset(); }

const void* fr_profile_json(void) {
    return json_call([&]() {
        Value a = Value::array();
        for (const auto& s : frdev::profile_stats()) {
            Value o = Value::object();
            o.set("kernel", Value::string(s.name));
            o.set("launches", Value::uint(s.launches));
            o.set("total_ms", Value::number(s.total_ms));
            a.push(std::move(o));
        }
        return frjson::dump(a);
    });
}

int fr_synchronize(void) {
    std::string err;
    return frdev::device_synchronize(&err) ? 0 : 1;
}

}  // extern "C"
