// ---------------------------------------------------------------------------------------------
// Model explanation (DESIGN.md section 12; csrc/explain_host.hpp, explain.hip)
// ---------------------------------------------------------------------------------------------
extern "C" {

namespace {

// the documents of a view as explain.hip's kernels visit them
frdev::ExDocs explain_docs(fr::DatasetView& view) {
    frdev::DeviceDataset::TileForm tf;
    std::string err;
    if (!view.device().tile_form(&tf, &err)) fr::fail_str(err);
    if (tf.nonfinite) fr::fail_str("explain: the dataset holds inf or NaN feature values");
    frdev::ExDocs docs;
    docs.xb = tf.xb, docs.dq = (uint32_t)tf.dq, docs.d = (uint32_t)tf.d, docs.device = tf.device;
    docs.pos.reserve(tf.n), docs.ids.reserve(tf.n);
    for (size_t p = 0; p < tf.np; p++)
        if (tf.perm_host[p] != 0xFFFFFFFFu) docs.pos.push_back((uint32_t)p), docs.ids.push_back(tf.perm_host[p]);
    return docs;
}

// bytes of device memory an explanation's output may take: what is free less a margin, or FR_EXPLAIN_MAX_BYTES if smaller
size_t explain_budget() {
    const size_t free_b = frdev::device_free_bytes(), margin = (size_t)256 << 20;
    size_t budget = free_b > margin ? free_b - margin : 0;
    if (free_b == 0) budget = std::numeric_limits<size_t>::max();  // (unknown)
    if (const char* e = std::getenv("FR_EXPLAIN_MAX_BYTES")) budget = std::min<size_t>(budget, (size_t)std::strtoull(e, nullptr, 10));
    return budget;
}

struct ExplainJob {
    fr::ExplainModel em;
    fr::ExplainPlan plan;
    frdev::ExDocs docs;
    std::vector<uint32_t> view_feats;  // the dataset's feature ids, ascending: the output's columns
    std::vector<int64_t> out_col;      // model feature -> output column, -1: a feature the dataset does not hold (phi = 0.0)
    frdev::ExTimes cover_t;
};

// everything up to the launch: the model's check (before any device is touched), the background's covers, the path table
ExplainJob explain_prepare(const CModel& m, const CDataset& ds, const CDataset* bg) {
    ExplainJob job;
    job.em = fr::explain_model(m.actual);
    fr::DatasetView& view = *ds.view;
    fr::DatasetView& bview = bg ? *bg->view : view;
    if (bview.instances.empty()) fr::fail_str("explain: the background dataset holds no instance");
    job.view_feats = features_ascending(view);
    if (view.instances.empty()) return job;
    job.docs = explain_docs(view);
    for (uint32_t f : job.em.feats) {
        const auto it = std::lower_bound(job.view_feats.begin(), job.view_feats.end(), f);
        const bool listed = it != job.view_feats.end() && *it == f;
        if (!listed && f < job.docs.d)
            fr::fail_str("explain: the model splits on feature " + std::to_string(f) + ", which the dataset's matrix holds but this feature sample does not list");
        job.out_col.push_back(listed ? (int64_t)(it - job.view_feats.begin()) : -1);
    }
    const frdev::ExWalk walk = fr::explain_walk(job.em);
    std::vector<uint32_t> counts;
    std::string err;
    if (&bview == &view) {
        if (!frdev::explain_covers(job.docs, walk, &counts, &job.cover_t, &err)) fr::fail_str(err);
    } else {
        const frdev::ExDocs bdocs = explain_docs(bview);
        if (bdocs.device != job.docs.device) fr::fail_str("explain: the background dataset lives on another device");
        if (!frdev::explain_covers(bdocs, walk, &counts, &job.cover_t, &err)) fr::fail_str(err);
    }
    job.plan = fr::explain_plan(job.em, counts, job.docs.d);
    return job;
}

Value explain_status(const ExplainJob& job, const frdev::ExTimes& t) {
    Value o = Value::object(), ids = Value::array(), sc = Value::array();
    for (uint32_t f : job.view_feats) ids.push(Value::uint(f));
    std::vector<uint64_t> counts(job.view_feats.size(), 0);
    for (size_t k = 0; k < job.out_col.size(); k++)
        if (job.out_col[k] >= 0) counts[(size_t)job.out_col[k]] = job.em.split_counts[k];
    for (uint64_t c : counts) sc.push(Value::uint(c));
    o.set("feature_ids", std::move(ids));
    o.set("split_counts", std::move(sc));
    o.set("expected_value", Value::number(job.plan.bias));
    o.set("trees", Value::uint(job.em.trees.size()));
    o.set("leaf_paths", Value::uint(job.plan.tab.value.size()));
    o.set("max_path", Value::uint(job.plan.tab.max_path));
    o.set("documents", Value::uint(job.docs.pos.size()));
    o.set("cover_ms", Value::number(job.cover_t.kernel_ms));
    o.set("kernel_ms", Value::number(t.kernel_ms));
    o.set("copy_ms", Value::number(t.copy_ms));
    return o;
}

}  // namespace

const void* fr_explain_dense(const CModel* model, const CDataset* dataset, const CDataset* background_or_null, double* out, size_t rows, size_t cols) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        DatasetLocks lk(ds, background_or_null);
        ExplainJob job = explain_prepare(m, ds, background_or_null);
        const size_t nf = job.view_feats.size();
        if (cols != nf + 1) fr::fail_str("fr_explain_dense: the dataset has " + std::to_string(nf) + " features, so cols must be " + std::to_string(nf + 1) + " (the bias comes last)");
        if (rows && !out) fr::fail_str("NULL pointer: fr_explain_dense out");
        frdev::ExTimes t;
        if (!job.docs.pos.empty()) {
            std::vector<double> phi;
            std::string err;
            if (!frdev::explain_values(job.docs, job.plan.tab, explain_budget(), &phi, &t, &err)) fr::fail_str(err);
            const size_t nc = job.plan.tab.ncols;
            for (size_t i = 0; i < job.docs.ids.size(); i++) {
                const size_t id = job.docs.ids[i];
                if (id >= rows) continue;
                double* row = out + id * cols;
                std::fill(row, row + nf, 0.0);
                for (size_t c = 0; c < nc; c++)
                    if (job.out_col[c] >= 0) row[job.out_col[c]] = phi[i * nc + c];
                row[nf] = job.plan.bias;
            }
        }
        return frjson::dump(explain_status(job, t));
    });
}

const void* fr_feature_importance(const CModel* model, const CDataset* dataset, const CDataset* background_or_null, double* out_mean_abs, size_t n_features) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        DatasetLocks lk(ds, background_or_null);
        ExplainJob job = explain_prepare(m, ds, background_or_null);
        const size_t nf = job.view_feats.size();
        if (n_features != nf) fr::fail_str("fr_feature_importance: the dataset has " + std::to_string(nf) + " features, n_features is " + std::to_string(n_features));
        if (nf && !out_mean_abs) fr::fail_str("NULL pointer: fr_feature_importance out_mean_abs");
        if (job.docs.pos.empty()) fr::fail_str("fr_feature_importance: the dataset holds no instance");
        frdev::ExTimes t;
        std::vector<double> sums;
        std::string err;
        if (!frdev::explain_sum_abs(job.docs, job.plan.tab, &sums, &t, &err)) fr::fail_str(err);
        std::fill(out_mean_abs, out_mean_abs + nf, 0.0);
        const double n = (double)job.docs.pos.size();
        for (size_t c = 0; c < sums.size(); c++)
            if (job.out_col[c] >= 0) out_mean_abs[job.out_col[c]] = sums[c] / n;
        return frjson::dump(explain_status(job, t));
    });
}

}  // extern "C"
