// extern "C" boundary of libfastrank_amd.so -- see include/fastrank.h for the contract and the
// reference file:line each symbol replaces (src/lib.rs, src/ffi.rs, src/json_api.rs).
#include <atomic>
#include <limits>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "../../include/fastrank.h"
#include "host.hpp"
#include "loader.hpp"
#include "explain_host.hpp"
#include "normalize_host.hpp"
#include "resample_host.hpp"
#include "permute_host.hpp"
#include "forest_pack.hpp"
#include "lambdamart.hpp"
#include "rf_train.hpp"
#include "verify_end.hpp"

using fr::FrError;
using frjson::Value;

struct CDataset {
    std::shared_ptr<fr::DatasetView> view;
};
struct CModel {
    fr::Model actual;
};
struct CQRel {
    fr::QRel actual;
};

// The parts of this translation unit (DESIGN.md section 2 lists what each holds): shared plumbing first, then every
// group of extensions, the test hooks last.  What follows them here is the reference's own surface, in src/lib.rs order.
#include "capi_support.inc"
#include "capi_train.inc"
#include "capi_evaluate.inc"
#include "capi_explain.inc"
#include "capi_normalize.inc"
#include "capi_compare.inc"
#include "capi_permute.inc"
#include "capi_debug.inc"
#include "capi_debug_trees.inc"

namespace {

Value random_forest_defaults_json() {
    // src/random_forest.rs:141-157 (+ :14-20 tuple-variant wire form {"SquaredError":[]})
    fr::Rand64 rand(0xdeadbeefULL);
    Value p = Value::object();
    p.set("seed", Value::uint(rand.rand_u64()));
    p.set("quiet", Value::boolean(false));
    p.set("num_trees", Value::uint(100));
    p.set("weight_trees", Value::boolean(false));
    Value sm = Value::object();
    sm.set("SquaredError", Value::array());
    p.set("split_method", std::move(sm));
    p.set("instance_sampling_rate", Value::number(0.5));
    p.set("feature_sampling_rate", Value::number(0.25));
    p.set("min_leaf_support", Value::uint(10));
    p.set("split_candidates", Value::uint(3));
    p.set("max_depth", Value::uint(8));
    return p;
}

// Rust's Display for f64: shortest round-trip digits, never exponent form
std::string rust_display_f64(double v) {
    if (v != v) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::scientific);
    std::string sci(buf, r.ptr);
    bool neg = sci[0] == '-';
    if (neg) sci.erase(0, 1);
    size_t epos = sci.find('e');
    std::string digits;
    for (char c : sci.substr(0, epos))
        if (c != '.') digits += c;
    int exp10 = atoi(sci.c_str() + epos + 1);
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    std::string out = neg ? "-" : "";
    int kk = exp10 + 1;
    if (digits == "0") return out + "0";
    if (kk <= 0) {
        out += "0.";
        out.append((size_t)(-kk), '0');
        out += digits;
    } else if ((int)digits.size() <= kk) {
        out += digits;
        out.append((size_t)(kk - (int)digits.size()), '0');
    } else {
        out.append(digits, 0, (size_t)kk);
        out += '.';
        out.append(digits, (size_t)kk, std::string::npos);
    }
    return out;
}

}  // namespace

extern "C" {

void free_str(void* p) { free(p); }
void free_c_result(CResult* p) { free(p); }
void free_dataset(CDataset* p) { delete p; }
void free_model(CModel* p) { delete p; }
void free_cqrel(CQRel* p) { delete p; }

const CResult* load_cqrel(const void* data_path) {
    return c_call<CQRel>([&]() {
        std::string path = accept_str("data_path", data_path);
        return new_handle<CQRel>([&] { return fr::load_qrel_file(path); });
    });
}

const CResult* cqrel_from_json(const void* json_str) {
    return c_call<CQRel>([&]() {
        Value v = parse_json_or_fail(accept_str("json_str", json_str));
        return new_handle<CQRel>([&] { return fr::qrel_from_json(v); });
    });
}

const void* cqrel_query_json(const CQRel* cqrel, const void* query_str) {
    return json_call([&]() {
        if (!cqrel) fr::fail_str("cqrel pointer is null!");
        std::string cmd = accept_str("query_str", query_str);
        if (cmd == "to_json") return frjson::dump(fr::qrel_to_json(cqrel->actual));
        if (cmd == "queries") {
            Value a = Value::array();
            for (const auto& q : cqrel->actual.queries) a.push(Value::string(q.first));
            return frjson::dump(a);
        }
        const auto* docs = cqrel->actual.get(cmd);
        if (!docs) fr::fail_str("Unknown request: " + cmd);
        return frjson::dump(fr::qrel_query_to_json(*docs));
    });
}

const CResult* load_ranksvm_format(void* data_path, void* feature_names_path) { return fr_load_ranksvm(data_path, feature_names_path, "auto"); }

const CResult* dataset_query_sampling(CDataset* dataset, const void* queries_json_list) {
    return c_call<CDataset>([&]() {
        const CDataset& ds = require_dataset(dataset);
        Value v = parse_json_or_fail(accept_str("queries_json_list", queries_json_list));
        if (!v.is_array()) fr::fail_raw("Error(\"invalid type: expected a sequence\", line: 1, column: 1)");
        std::set<std::string> wanted;
        for (const auto& x : v.arr) {
            if (!x.is_string()) fr::fail_raw("Error(\"invalid type: expected a string\", line: 1, column: 1)");
            wanted.insert(x.s);
        }
        // src/sampling.rs:117-133 with_queries
        auto child = std::make_shared<fr::DatasetView>();
        child->core = ds.view->core;
        child->features = ds.view->features;
        child->sampled = true;
        child->parent = ds.view;
        for (auto& qi : instances_by_query(*ds.view))
            if (wanted.count(qi.first)) child->instances.insert(child->instances.end(), qi.second.begin(), qi.second.end());
        auto* out = new CDataset();
        out->view = child;
        return out;
    });
}

const CResult* dataset_feature_sampling(CDataset* dataset, const void* feature_json_list) {
    return c_call<CDataset>([&]() {
        const CDataset& ds = require_dataset(dataset);
        Value v = parse_json_or_fail(accept_str("feature_json_list", feature_json_list));
        if (!v.is_array()) fr::fail_raw("Error(\"invalid type: expected a sequence\", line: 1, column: 1)");
        // src/sampling.rs:91-115 with_features
        std::set<uint32_t> valid(ds.view->features.begin(), ds.view->features.end());
        std::set<uint32_t> keep, missing;
        for (const auto& x : v.arr) {
            uint32_t fid = (uint32_t)fr::json_u64(x, "FeatureId");
            (valid.count(fid) ? keep : missing).insert(fid);
        }
        if (!missing.empty()) {
            std::string s = "Missing Features: {";
            bool first = true;
            for (uint32_t f : missing) {
                if (!first) s += ", ";
                s += "FeatureId(" + std::to_string(f) + ")";
                first = false;
            }
            fr::fail_str(s + "}");
        }
        if (keep.empty()) fr::fail_str("No Features!");
        auto child = std::make_shared<fr::DatasetView>();
        child->core = ds.view->core;
        child->features.assign(keep.begin(), keep.end());
        child->instances = ds.view->instances;
        child->sampled = true;
        child->parent = ds.view;
        child->same_instances_as_parent = true;
        auto* out = new CDataset();
        out->view = child;
        return out;
    });
}

const void* dataset_query_json(void* dataset, void* json_cmd_str) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        const fr::DatasetView& v = *ds.view;
        std::string cmd = accept_str("dataset_query_json", json_cmd_str);
        // src/ffi.rs:144-183
        if (cmd == "is_sampled") return std::string(v.sampled ? "true" : "false");
        if (cmd == "num_features") return std::to_string(v.n_dim());
        if (cmd == "feature_ids") {
            Value a = Value::array();
            for (uint32_t f : v.features) a.push(Value::uint(f));
            return frjson::dump(a);
        }
        if (cmd == "num_instances") return std::to_string(v.instances.size());
        if (cmd == "queries") {
            Value a = Value::array();
            for (auto& qi : instances_by_query(v)) a.push(Value::string(qi.first));
            return frjson::dump(a);
        }
        if (cmd == "instances_by_query") {
            Value o = Value::object();
            for (auto& qi : instances_by_query(v)) {
                Value a = Value::array();
                for (uint32_t id : qi.second) a.push(Value::uint(id));
                o.obj.emplace_back(qi.first, std::move(a));
            }
            return frjson::dump(o);
        }
        if (cmd == "feature_names") {
            Value a = Value::array();
            for (uint32_t f : v.features) a.push(Value::string(v.core->feature_name(f)));
            return frjson::dump(a);
        }
        // the normaliser a dataset made by fr_normalize_dataset remembers (null for any other), and what making it took
        if (cmd == "normalization" || cmd == "normalization_stats") {
            const NormMemo memo = norm_memo_of(v.core);
            const std::string& text = cmd == "normalization" ? memo.normalization : memo.stats;
            return text.empty() ? std::string("null") : text;
        }
        return frjson::dump(unknown_cmd("unknown_dataset_query_str", cmd));
    });
}

const void* query_json(const void* json_cmd_str) {
    return json_call([&]() {
        std::string cmd = accept_str("query_json_str", json_cmd_str);
        // src/ffi.rs:215-236
        if (cmd == "coordinate_ascent_defaults" || cmd == "random_forest_defaults" || cmd == "lambdamart_defaults") {
            Value o = Value::object();
            o.set("measure", Value::string("ndcg"));
            Value params = Value::object();
            if (cmd == "coordinate_ascent_defaults")
                params.set("CoordinateAscent", fr::CAParams::defaults().to_json());
            else if (cmd == "lambdamart_defaults")
                params.set("LambdaMART", fr::LambdaMARTParams().to_json());
            else
                params.set("RandomForest", random_forest_defaults_json());
            o.set("params", std::move(params));
            o.set("judgments", Value::null());
            return frjson::dump(o);
        }
        if (cmd == "measures") {  // the evaluators every call takes by name (measures_host.hpp)
            Value a = Value::array();
            const frmeasure::MeasureInfo* t = frmeasure::measure_table();
            for (int i = 0; i < frmeasure::MEASURE_COUNT; i++) {
                Value o = Value::object();
                o.set("name", Value::string(t[i].names[0]));
                Value al = Value::array();
                if (t[i].names[1] != nullptr) al.push(Value::string(t[i].names[1]));
                o.set("aliases", std::move(al));
                o.set("display", Value::string(t[i].display));
                o.set("cutoff", Value::string(frmeasure::cutoff_name(t[i].cutoff)));
                a.push(std::move(o));
            }
            return frjson::dump(a);
        }
        return frjson::dump(unknown_cmd("unknown_query_str", cmd));
    });
}

const CResult* make_dense_dataset_f32_f64_i64(size_t n, size_t d, const float* x, const double* y,
                                              const int64_t* qids) {
    return c_call<CDataset>([&]() {
        if ((n && (!x || !y || !qids))) fr::fail_str("NULL pointer: dense dataset arrays");
        return new_handle<CDataset>([&] { return fr::make_dense(n, d, x, y, qids); });
    });
}

const CResult* train_model(void* train_request_json, void* dataset) {
    return c_call<CModel>([&]() {
        // src/lib.rs:249-252: the dataset pointer is checked after the request is parsed lazily;
        // result_train_model reports the null dataset first (src/ffi.rs:189-193)
        const CDataset& ds = require_dataset(dataset);
        ParsedRequest rq = parse_train_request(accept_str("train_request_json", train_request_json));
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        return new_model([&] {
            switch (rq.learner) {
                case Learner::CoordinateAscent: return train_ca_devices(ds.view, rq);
                case Learner::RandomForest: return train_rf(ds.view, rq);
                case Learner::LambdaMART: break;
            }
            return train_lambdamart(ds.view, rq);
        });
    });
}

const CResult* model_from_json(const void* json_str) {
    return c_call<CModel>([&]() {
        Value v = parse_json_or_fail(accept_str("json_str", json_str));
        return new_model([&] { return fr::model_from_json(v); });
    });
}

const void* model_query_json(const void* model, const void* json_cmd_str) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        std::string cmd = accept_str("query_json", json_cmd_str);
        if (cmd == "to_json") return frjson::dump(fr::model_to_json(m.actual));
        return frjson::dump(unknown_cmd("unknown_dataset_query_str", cmd));  // sic: src/ffi.rs:206-209
    });
}

const void* evaluate_by_query(const CModel* model, const CDataset* dataset, const CQRel* qrel,
                              const void* evaluator) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::string name = accept_str("evaluator_name", evaluator);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        fr::Evaluator ev = fr::make_evaluator(view, name, qrel ? &qrel->actual : nullptr);
        Value o = Value::object();
        if (view.instances.empty()) return frjson::dump(o);
        frdev::DeviceDataset& dev = view.device();
        fr::score_model(view, m.actual);
        evaluate_scores(dev, ev, 1);
        std::string err;
        std::vector<double> vals(dev.nq());
        if (!dev.download_per_query(1, vals.data(), &err)) fr::fail_str(err);
        for (size_t q = 0; q < vals.size(); q++)
            o.obj.emplace_back(view.core->qnames[view.csr_query[q]], Value::number(vals[q]));
        return frjson::dump(o);
    });
}

const void* predict_scores(const CModel* model, const CDataset* dataset) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) return std::string("{}");
        frdev::DeviceDataset& dev = view.device();
        fr::score_model(view, m.actual);
        std::vector<double> scores(view.core->n, 0.0);
        std::string err;
        if (!dev.download_scores(0, scores.data(), scores.size(), &err)) fr::fail_str(err);
        for (uint32_t id : view.instances)
            if (scores[id] != scores[id]) fr::fail_str("Model.predict -> NaN");
        // src/json_api.rs:53-72: {"<instance index>": score}
        std::string out = "{";
        bool first = true;
        std::vector<uint32_t> ids = view.instances;
        std::sort(ids.begin(), ids.end());
        for (uint32_t id : ids) {
            if (!first) out += ',';
            first = false;
            out += '"';
            out += std::to_string(id);
            out += "\":";
            frjson::write_double(out, scores[id]);
        }
        out += '}';
        return out;
    });
}

const void* predict_to_trecrun(const CModel* model, const CDataset* dataset, const void* output_path,
                               const void* system_name, size_t depth) {
    return json_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::string path = accept_str("output_path", output_path);
        std::string sysname = accept_str("system_name", system_name);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        // src/json_api.rs:75-120
        std::ofstream out(path);
        if (!out) fr::fail_str("could not open " + path + " for writing");
        size_t written = 0;
        if (view.instances.empty()) return std::to_string(written);
        frdev::DeviceDataset& dev = view.device();
        rank_view(view, m.actual);
        std::string err;
        std::vector<uint32_t> rank(dev.n());
        if (!dev.download_rank(rank.data(), &err)) fr::fail_str(err);
        std::vector<double> scores(view.core->n, 0.0);
        if (!dev.download_scores(0, scores.data(), scores.size(), &err)) fr::fail_str(err);
        const frdev::HostCSR& csr = view.host_csr();
        const fr::DataCore& c = *view.core;
        for (size_t q = 0; q < csr.nq; q++) {
            const std::string& qid = c.qnames[view.csr_query[q]];
            for (uint32_t p = csr.qoff[q]; p < csr.qoff[q + 1]; p++) {
                size_t rk = p - csr.qoff[q] + 1;
                if (depth > 0 && rk > depth) break;
                uint32_t id = rank[p];
                if (!c.has_docids || id >= c.doc_present.size() || !c.doc_present[id])
                    fr::fail_str("Dataset does not contain document ids and therefore cannot save to trecrun!");
                out << qid << " Q0 " << c.docids[id] << " " << rk << " " << rust_display_f64(scores[id]) << " "
                    << sysname << "\n";
                written++;
            }
            out.flush();
        }
        return std::to_string(written);
    });
}

}  // extern "C"
