// ---------------------------------------------------------------------------------------------
// Feature normalisation (DESIGN.md section 14; csrc/normalize_host.hpp, normalize.hip)
// ---------------------------------------------------------------------------------------------
namespace {

// What fr_normalize_dataset remembers of the datasets it made: the normaliser's JSON (a second one is refused) and what
// making the dataset took.  Kept beside DataCore, not in it: host.hpp is one of device.o's sources, and a dataset that was
// never normalised has nothing here.  Entries of cores that are gone are dropped at the next insert.
struct NormMemo {
    std::string normalization, stats;
};
std::mutex g_norm_mu;
std::vector<std::pair<std::weak_ptr<fr::DataCore>, NormMemo>> g_norm_memo;
NormMemo norm_memo_of(const std::shared_ptr<fr::DataCore>& core) {
    std::lock_guard<std::mutex> lk(g_norm_mu);
    for (const auto& e : g_norm_memo)
        if (e.first.lock() == core) return e.second;
    return NormMemo();
}
void norm_memo_set(const std::shared_ptr<fr::DataCore>& core, NormMemo memo) {
    std::lock_guard<std::mutex> lk(g_norm_mu);
    g_norm_memo.erase(std::remove_if(g_norm_memo.begin(), g_norm_memo.end(), [](const auto& e) { return e.first.expired(); }), g_norm_memo.end());
    g_norm_memo.emplace_back(core, std::move(memo));
}

}  // namespace

extern "C" {

namespace {

// the instances `list` of a view (its iteration order, or a regrouping of it) as normalize.hip's kernels visit them
frdev::NormDocs normalize_docs(fr::DatasetView& view, const std::vector<uint32_t>& list) {
    frdev::DeviceDataset::TileForm tf;
    std::string err;
    if (!view.device().tile_form(&tf, &err)) fr::fail_str(err);
    const fr::DataCore& c = *view.core;
    frdev::NormDocs docs;
    docs.xb = tf.xb, docs.dq = (uint32_t)tf.dq, docs.d = (uint32_t)tf.d, docs.device = tf.device;
    std::vector<uint32_t> at(c.n, 0xFFFFFFFFu);
    for (size_t p = 0; p < tf.np; p++)
        if (tf.perm_host[p] != 0xFFFFFFFFu && tf.perm_host[p] < c.n) at[tf.perm_host[p]] = (uint32_t)p;
    docs.pos.reserve(list.size());
    for (uint32_t id : list) {
        if (id >= c.n || at[id] == 0xFFFFFFFFu) fr::fail_str("normalisation: instance " + std::to_string(id) + " has no place in the dataset's device form");
        docs.pos.push_back(at[id]);
    }
    docs.ids = list;
    if (!c.present_bits.empty()) docs.present = c.present_bits.data(), docs.present_words = c.present_words, docs.core_n = c.n;
    docs.fmask.assign((docs.d + 31) / 32, 0u);
    for (uint32_t f : view.features)
        if (f < docs.d) docs.fmask[f >> 5] |= 1u << (f & 31u);
    return docs;
}

[[noreturn]] void normalize_fail_stat(uint64_t cell) {
    fr::fail_str("non-finite value in feature " + std::to_string(cell & 0xFFFFFFFFu) + ", instance " + std::to_string(cell >> 32) +
                 ": feature statistics need finite values");
}

}  // namespace

const void* fr_fit_normalizer(const CDataset* dataset, const void* method) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        fr::Normalizer nm;
        nm.kind = fr::norm_method(accept_str("method", method));
        if (nm.kind == fr::Normalizer::Sigmoid) return frjson::dump(fr::norm_to_json(nm));
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) return frjson::dump(fr::norm_to_json(nm));
        const frdev::NormDocs docs = normalize_docs(view, view.instances);
        std::vector<frdev::NormRecord> records;
        uint64_t bad = frdev::NORM_NO_CELL;
        std::string err;
        if (!frdev::normalize_stats(docs, &records, &bad, nullptr, &err)) fr::fail_str(err);
        if (bad != frdev::NORM_NO_CELL) normalize_fail_stat(bad);
        for (uint32_t f : view.features) {
            fr::ComputedStats cs;
            if (f < docs.d && fr::norm_finish(records[f], &cs)) nm.stats[f] = cs;
        }
        return frjson::dump(fr::norm_to_json(nm));
    });
}

const CResult* fr_normalize_dataset(const CDataset* dataset, const void* normalizer_json) {
    return c_call<CDataset>([&]() {
        const CDataset& ds = require_dataset(dataset);
        const fr::Normalizer nm = fr::norm_from_json(parse_json_or_fail(accept_str("normalizer_json", normalizer_json)));
        fr::DatasetView& view = *ds.view;
        const fr::DataCore& c = *view.core;
        if (view.sampled || view.instances.size() != c.n) fr::fail_str("normalise the whole dataset, then sample it");
        if (!norm_memo_of(view.core).normalization.empty()) fr::fail_str("Cannot apply normalization twice!");
        if (c.n == 0 || c.d == 0) fr::fail_str("normalisation: the dataset holds no instance");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> list(c.n);
        std::vector<uint32_t> qoff;
        if (nm.per_query()) {  // the queries' instances in the view's order, query after query (instances_by_query)
            std::vector<uint32_t> count(c.qnames.size(), 0);
            for (uint32_t id : view.instances) count[c.qix[id]]++;
            std::vector<uint32_t> start(c.qnames.size() + 1, 0);
            for (size_t q = 0; q < count.size(); q++) start[q + 1] = start[q] + count[q];
            std::vector<uint32_t> fill(start.begin(), start.end() - 1);
            for (uint32_t id : view.instances) list[fill[c.qix[id]]++] = id;
            for (size_t q = 0; q < count.size(); q++)
                if (count[q]) qoff.push_back(start[q]);
            qoff.push_back((uint32_t)c.n);
        } else {
            for (size_t i = 0; i < c.n; i++) list[i] = (uint32_t)i;
        }
        const frdev::NormDocs docs = normalize_docs(view, list);
        if (docs.d != c.d) fr::fail_str("normalisation: the device form holds " + std::to_string(docs.d) + " columns, the dataset " + std::to_string(c.d));
        const auto t_docs = std::chrono::steady_clock::now();
        auto core = std::make_shared<fr::DataCore>();
        core->x_own.resize(c.n * c.d);
        const auto t_alloc = std::chrono::steady_clock::now();
        frdev::NormTimes times;
        uint64_t bad = frdev::NORM_NO_CELL, bad_stat = frdev::NORM_NO_CELL;
        std::string err;
        if (nm.per_query()) {
            if (!frdev::normalize_per_query(docs, qoff, nm.kind == fr::Normalizer::PerQueryMaxMin ? frdev::NORM_M_MAXMIN : frdev::NORM_M_ZSCORE,
                                            core->x_own.data(), &bad_stat, &bad, &times, &err))
                fr::fail_str(err);
        } else {
            if (!frdev::normalize_apply(docs, fr::norm_params(nm, c.d), core->x_own.data(), &bad, &times, &err)) fr::fail_str(err);
        }
        if (bad_stat != frdev::NORM_NO_CELL) normalize_fail_stat(bad_stat);
        if (bad != frdev::NORM_NO_CELL)
            fr::fail_str(std::string("Normalization.") + nm.method() + " NaN: feature " + std::to_string(bad & 0xFFFFFFFFu) + ", instance " + std::to_string(bad >> 32));
        const auto t1 = std::chrono::steady_clock::now();
        core->n = c.n, core->d = c.d, core->x = core->x_own.data();
        core->gain = c.gain, core->qix = c.qix, core->qnames = c.qnames;
        core->has_docids = c.has_docids, core->docids = c.docids, core->doc_present = c.doc_present;
        core->features = c.features, core->feature_names = c.feature_names;
        core->present_bits = c.present_bits, core->present_words = c.present_words;
        auto* out = new CDataset();
        out->view = std::make_shared<fr::DatasetView>();
        out->view->core = core;
        out->view->features = view.features;
        out->view->instances = view.instances;
        // where the call's time went: the list and its positions; the new matrix's host memory; on the device the kernel, the
        // download and the rest (buffers, the list's upload); the new core's other fields
        const auto secs = [](auto a, auto b) { return std::chrono::duration<double>(b - a).count(); };
        const auto t2 = std::chrono::steady_clock::now();
        Value st = Value::object();
        st.set("prepare_seconds", Value::number(secs(t0, t_docs)));
        st.set("allocate_seconds", Value::number(secs(t_docs, t_alloc)));
        st.set("kernel_seconds", Value::number(times.kernel_ms * 1e-3));
        st.set("download_seconds", Value::number(times.copy_ms * 1e-3));
        st.set("device_other_seconds", Value::number(secs(t_alloc, t1) - (times.kernel_ms + times.copy_ms) * 1e-3));
        st.set("core_build_seconds", Value::number(secs(t1, t2)));
        st.set("total_seconds", Value::number(secs(t0, t2)));
        norm_memo_set(core, NormMemo{frjson::dump(fr::norm_to_json(nm)), frjson::dump(st)});
        return out;
    });
}

}  // extern "C"
