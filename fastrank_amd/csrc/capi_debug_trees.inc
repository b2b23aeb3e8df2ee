// capi.cpp: the test hooks of the tree trainers -- LambdaMART's samples, DART plan and gradients, the histogram grower and
// what it is built from (bins, GOSS, quantised gradients, the root histogram), the random forest's recorded levels.
extern "C" {

// per query of the view (its order) whether `queries` names it
static std::vector<unsigned char> debug_query_flags(const uint32_t* queries, size_t n_queries, size_t nq) {
    if (n_queries == 0) fr::fail_str("a query sample must name at least one query");
    std::vector<unsigned char> flags(nq, 0);
    for (size_t i = 0; i < n_queries; i++) {
        if (queries[i] >= nq) fr::fail_str("a query sample names query " + std::to_string(queries[i]) + " of " + std::to_string(nq));
        flags[queries[i]] = 1;
    }
    return flags;
}

// The sample LambdaMART's trainer uses for tree `tree` of the request parameters `params_json` ({"num_trees": ..}, the
// LambdaMART variant's payload) on this view: {"features": [ids ascending], "queries": [indices in the view's order]}; with
// validation_queries these are the sampled TRAINING queries.
// No device is touched.
const void* fr_debug_lambdamart_sample(const CDataset* dataset, const void* params_json, uint32_t tree) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        const fr::LambdaMARTParams p = fr::LambdaMARTParams::from_json(parse_json_or_fail(accept_str("params_json", params_json)));
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        const std::vector<uint32_t> feats = features_ascending(view);
        const size_t nq = view.host_csr().nq;
        const fr::LambdaSplit split = fr::lambdamart_split(view, p);  // (held-out queries: the sample is drawn from the others)
        fr::Rand64 master(p.seed);
        fr::LambdaSample smp;
        for (uint32_t t = 0; t <= tree; t++) smp = fr::lambdamart_next_sample(master, feats.size(), nq, p, split.held.empty() ? nullptr : &split.train);
        Value o = Value::object(), f = Value::array(), q = Value::array();
        for (uint32_t s : smp.features) f.push(Value::uint(feats[s]));
        for (uint32_t x : smp.queries) q.push(Value::uint(x));
        o.set("features", std::move(f));
        o.set("queries", std::move(q));
        return frjson::dump(o);
    });
}

// LambdaMART's DART plan (csrc/lambdamart_dart.hpp) for the first `num_trees` trees of the request parameters `params_json`
// (the LambdaMART variant's payload; its own num_trees is not read): [{"dropped": [tree indices ascending], "before": [the
// weights w_0 .. w_{t-1}], "after": [w_0 .. w_t]}, ...], one entry per tree.  No device is touched.
const void* fr_debug_lambdamart_dart_plan(const void* params_json, uint32_t num_trees) {
    return json_call([&]() {
        const fr::LambdaMARTParams p = fr::LambdaMARTParams::from_json(parse_json_or_fail(accept_str("params_json", params_json)));
        fr::DartPlan plan(p.seed, p.drop_rate, p.max_drop, p.skip_drop);
        std::vector<double> w;
        Value out = Value::array();
        auto numbers = [](const std::vector<double>& v) {
            Value a = Value::array();
            for (double x : v) a.push(Value::number(x));
            return a;
        };
        for (uint32_t t = 0; t < num_trees; t++) {
            const std::vector<uint32_t> dropped = p.dart() ? plan.next(t) : std::vector<uint32_t>();
            Value o = Value::object(), d = Value::array();
            for (uint32_t i : dropped) d.push(Value::uint(i));
            o.set("dropped", std::move(d));
            o.set("before", numbers(w));
            fr::dart_reweight(w, dropped, p.learning_rate);
            o.set("after", numbers(w));
            out.push(std::move(o));
        }
        return frjson::dump(out);
    });
}

// dart_rescore_kernel on its own: `model` must be an Ensemble of DecisionTrees (its own weights are not read).  The leaf cache
// is filled for its trees as the trainer fills it, then the scores s = sum over include[k] (ascending tree indices) of
// weights[include[k]] * tree(x) are formed once.  scores_out[out_len]: by instance id; cache_out[n_weights][out_len]: the
// cache's rows by instance id (entries of instances outside the dataset are left as they are).  n_weights = the number of trees.
const void* fr_debug_dart_scores(const CDataset* dataset, const CModel* model, const double* weights, size_t n_weights,
                                 const uint32_t* include, size_t n_include, double* scores_out, uint16_t* cache_out, size_t out_len) {
    return status_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        const fr::Model& ens = m.actual;
        bool trees = ens.kind == fr::Model::Ensemble && !ens.members.empty();
        for (const auto& mm : ens.members) trees = trees && mm.kind == fr::Model::DecisionTree;
        if (!trees) fr::fail_str("fr_debug_dart_scores: the model must be an Ensemble of DecisionTrees");
        if (n_weights != ens.members.size()) fr::fail_str("fr_debug_dart_scores: one weight per tree of the model");
        if ((n_weights && !weights) || (n_include && !include) || (out_len && (!scores_out || !cache_out)))
            fr::fail_str("NULL pointer: fr_debug_dart_scores");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) return;
        frdev::DeviceDataset& dev = view.device();
        std::string err;
        struct End {
            frdev::DeviceDataset& d;
            ~End() { d.dart_end(); }
        } end{dev};
        if (!dev.dart_begin(n_weights, nullptr, &err)) fr::fail_str(err);
        for (size_t t = 0; t < n_weights; t++) {
            std::vector<fr::TreeNode*> leaves;
            fr::Model rm;
            rm.kind = fr::Model::DecisionTree;
            rm.tree = fr::LambdaMARTTrainer::number_leaves(*ens.members[t].tree, leaves);
            fr::score_model(view, rm, &dev);
            std::vector<double> values(leaves.size());
            for (size_t L = 0; L < leaves.size(); L++) values[L] = leaves[L]->value;
            if (!dev.dart_fill(t, values.data(), values.size(), &err)) fr::fail_str(err);
        }
        if (!dev.dart_rescore(weights, n_weights, include, n_include, &err)) fr::fail_str(err);
        if (!dev.download_scores(0, scores_out, out_len, &err)) fr::fail_str(err);
        for (size_t t = 0; t < n_weights; t++)
            if (!dev.dart_download_row(t, cache_out + t * out_len, out_len, &err)) fr::fail_str(err);
    });
}

// The body of the three gradient hooks below: one gradient pass on the model's scores, downloaded by instance id.  queries ==
// NULL: every query (need_queries: refused); else only the named queries' instances are computed and written.  options_json:
// nullptr for a hook that takes no options, else the address of the caller's string (fr_debug_lambda_gradients_opts below).
static const void* lambda_gradients_debug(const CModel* model, const CDataset* dataset, const CQRel* qrel, const void* measure, double sigma,
                                          const uint32_t* queries, size_t n_queries, bool need_queries, const void* const* options_json,
                                          double* lambda_out, double* weight_out, size_t out_len) {
    return status_call([&]() {
        const CModel& m = require_model(model);
        const CDataset& ds = require_dataset(dataset);
        std::string name = accept_str("measure", measure);
        fr::lambdamart_check_measure(name);
        fr::LambdaMARTParams op;
        uint64_t xe_key = 0;
        if (options_json) {
            const Value opts = parse_json_or_fail(accept_str("options_json", *options_json));
            if (!opts.is_object()) fr::fail_raw("Error(\"invalid type: expected a map of gradient options\", line: 0, column: 0)");
            for (const auto& kv : opts.obj) {
                if (kv.first == "truncation_level") op.truncation_level = fr::json_u32(kv.second, "truncation_level");
                else if (kv.first == "lambda_norm") op.lambda_norm = fr::json_bool(kv.second, "lambda_norm");
                else if (kv.first == "objective") op.objective = fr::LambdaMARTParams::objective_from_json(kv.second);
                else if (kv.first == "xe_key") xe_key = fr::json_u64(kv.second, "xe_key");
                else fr::fail_raw("Error(\"unknown field `" + kv.first + "`, expected `truncation_level` or `lambda_norm`\", line: 0, column: 0)");
            }
            op.check_objective_options();  // (before any device work, as the request parser does)
        }
        if (out_len && (!lambda_out || !weight_out)) fr::fail_str("NULL pointer: gradient outputs");
        if (need_queries && !queries) fr::fail_str("NULL pointer: query sample");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) return;
        std::vector<unsigned char> flags;
        if (queries) flags = debug_query_flags(queries, n_queries, view.host_csr().nq);
        const unsigned char* fl = queries ? flags.data() : nullptr;
        fr::Evaluator ev = fr::make_evaluator(view, op.objective_measure() ? std::string(op.objective_measure()) : name, qrel ? &qrel->actual : nullptr);
        frdev::DeviceDataset& dev = view.device();
        fr::score_model(view, m.actual);
        std::string err;
        if (!dev.lambda_gradients(ev.norms.data(), ev.depth, sigma, op.pass(fl, false, xe_key), &err)) fr::fail_str(err);
        if (!dev.lambda_download(lambda_out, weight_out, out_len, &err, fl)) fr::fail_str(err);
    });
}

const void* fr_debug_lambda_gradients(const CModel* model, const CDataset* dataset, const CQRel* qrel, const void* measure,
                                      double sigma, double* lambda_out, double* weight_out, size_t out_len) {
    return lambda_gradients_debug(model, dataset, qrel, measure, sigma, nullptr, 0, false, nullptr, lambda_out, weight_out, out_len);
}

// fr_debug_lambda_gradients for a query sample: queries[n_queries] = indices of the view's queries (its order).  Only their
// instances are written.
const void* fr_debug_lambda_gradients_sampled(const CModel* model, const CDataset* dataset, const CQRel* qrel, const void* measure,
                                              double sigma, const uint32_t* queries, size_t n_queries, double* lambda_out,
                                              double* weight_out, size_t out_len) {
    return lambda_gradients_debug(model, dataset, qrel, measure, sigma, queries, n_queries, true, nullptr, lambda_out, weight_out, out_len);
}

// fr_debug_lambda_gradients under the objective's options (DESIGN.md section 11, "Truncation and normalisation"):
// options_json = {"truncation_level": u32, "lambda_norm": bool, "objective": "ndcg" | "map" | "mrr" | "xendcg", "xe_key": u64},
// every key optional (0 / false / "ndcg" / 0).  queries == NULL: the full pass; else the query sample of fr_debug_lambda_gradients_sampled.  With
// every option at its default this is the pass of the two other hooks.  `measure` must name NDCG whatever the objective;
// under "map" / "mrr" the norms are the AP / RR evaluator's (DESIGN.md section 11, "Objectives").  "objective": "xendcg" is
// the listwise pass (section 11, "Listwise objective") under the key "xe_key" (u64, default 0; read under "xendcg" only); it
// keeps the NDCG norms, reads neither sigma nor the measure's depth, and refuses truncation_level != 0 and lambda_norm.
const void* fr_debug_lambda_gradients_opts(const CModel* model, const CDataset* dataset, const CQRel* qrel, const void* measure,
                                           double sigma, const uint32_t* queries, size_t n_queries, const void* options_json,
                                           double* lambda_out, double* weight_out, size_t out_len) {
    return lambda_gradients_debug(model, dataset, qrel, measure, sigma, queries, n_queries, false, &options_json, lambda_out, weight_out, out_len);
}

// the histogram grower's inputs for a view: its instance list and their positions, its features ascending
static void hist_debug_lists(fr::DatasetView& view, std::vector<uint32_t>* ids, std::vector<uint32_t>* positions, std::vector<uint32_t>* feats) {
    *ids = fr::lambdamart_instance_list(view.host_csr());
    *feats = features_ascending(view);
    positions->resize(ids->size());
    std::string err;
    if (!view.device().rf_positions(*ids, positions->data(), &err)) fr::fail_str(err);
}

const void* fr_debug_hist_bins(const CDataset* dataset, uint32_t split_candidates, size_t n, size_t f, uint32_t* ids_out,
                               uint32_t* feats_out, float* edges_out, uint32_t* nedges_out, uint8_t* bins_out) {
    return status_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        if (!ids_out || !feats_out || !edges_out || !nedges_out || !bins_out) fr::fail_str("NULL pointer: bin outputs");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        std::vector<uint32_t> ids, positions, feats, nedges;
        hist_debug_lists(view, &ids, &positions, &feats);
        if (ids.size() != n || feats.size() != f) fr::fail_str("fr_debug_hist_bins: the view has " + std::to_string(ids.size()) + " instances and " + std::to_string(feats.size()) + " features");
        frdev::DeviceDataset& dev = view.device();
        std::string err;
        std::vector<float> edges;
        if (!dev.hist_bins(positions.data(), n, feats, split_candidates, nullptr, &err)) fr::fail_str(err);
        if (!dev.hist_edges(&edges, &nedges, &err)) fr::fail_str(err);
        if (!dev.hist_download_bins(bins_out, n * f, &err)) fr::fail_str(err);
        std::copy(ids.begin(), ids.end(), ids_out);
        std::copy(feats.begin(), feats.end(), feats_out);
        std::copy(edges.begin(), edges.end(), edges_out);
        std::copy(nedges.begin(), nedges.end(), nedges_out);
    });
}

// What the tree hook and the selection hook below share: the view's lists, a query sample (queries == NULL: every query) as
// flags with its instance count, and values by instance id gathered into instance-list order.
struct HistDebugInput {
    const frdev::HostCSR& csr;
    std::vector<uint32_t> ids, positions, feats;
    const bool sampled;
    std::vector<unsigned char> flags;  // [nq] when sampled
    size_t n_t;                        // the sample's instances
    HistDebugInput(fr::DatasetView& view, const uint32_t* queries, size_t n_queries) : csr(view.host_csr()), sampled(queries != nullptr) {
        hist_debug_lists(view, &ids, &positions, &feats);
        n_t = ids.size();
        if (!sampled) return;
        flags = debug_query_flags(queries, n_queries, csr.nq);
        n_t = 0;
        for (size_t q = 0; q < csr.nq; q++)
            if (flags[q]) n_t += csr.qoff[q + 1] - csr.qoff[q];
    }
    const unsigned char* query_flags() const { return sampled ? flags.data() : nullptr; }
    // The caller's values go to the device as they are, also outside the query sample: the grower must not read those.  An
    // id past len is refused (too_short) inside the sample only; so is, when not_finite is given, a value that is not finite.
    std::vector<double> gather(const double* values, size_t len, const std::string& too_short, const char* not_finite = nullptr) const {
        std::vector<double> out(ids.size(), 0.0);
        size_t g = 0;
        for (size_t q = 0; q < csr.nq; q++) {
            const bool read = !sampled || flags[q];
            for (size_t j = csr.qoff[q]; j < csr.qoff[q + 1]; j++, g++) {
                if (ids[g] >= len) {
                    if (!read) continue;
                    fr::fail_str(too_short);
                }
                out[g] = values[ids[g]];
                if (not_finite && read && !std::isfinite(out[g])) fr::fail_str(not_finite);
            }
        }
        return out;
    }
};
// A grower on the view's bins under the hook's sample (sel: its feature selection, or null).  The bins stay with the view: it
// leaves them without a sample when it goes, also when the hook fails.
struct HistDebugGrower {
    fr::HistGrower g;
    HistDebugGrower(fr::DatasetView& view, const HistDebugInput& in, const fr::HistGrowOptions& grow, const std::vector<uint32_t>* sel = nullptr)
        : g(view.device(), in.feats, grow) {
        g.prepare(in.positions);
        try {
            g.set_sample(in.query_flags(), (uint32_t)in.n_t, sel);
        } catch (...) {
            unsample();
            throw;
        }
    }
    ~HistDebugGrower() { unsample(); }
    void unsample() {
        try {
            g.set_sample(nullptr, 0, nullptr);
        } catch (...) {
        }
    }
};
// (for a hook that reads no bin: the smallest bin matrix there is keeps it cheap on a view that has none yet)
static const fr::HistGrowOptions HIST_DEBUG_SMALLEST{2u, 1u, 1u, fr::HistNewton{true, 0.0, 0.0, 0.0}, 0u, {}};

// `features` as indices into feats (the view's, ascending), ascending; one the view does not hold, or one named twice, is refused
static std::vector<uint32_t> hist_debug_selection(const std::string& who, const std::vector<uint32_t>& feats, const uint32_t* features, size_t n_features) {
    std::vector<uint32_t> want(features, features + n_features), sel;
    std::sort(want.begin(), want.end());
    for (size_t i = 0; i < want.size(); i++) {
        const auto it = std::lower_bound(feats.begin(), feats.end(), want[i]);
        if (it == feats.end() || *it != want[i] || (i > 0 && want[i] == want[i - 1]))
            fr::fail_str(who + ": feature " + std::to_string(want[i]) + " is not in the view, or is named twice");
        sel.push_back((uint32_t)(it - feats.begin()));
    }
    return sel;
}

// the two GOSS rates as a debug hook takes them: the request parser's ranges, and top_rate > 0
static bool goss_debug_rates_ok(double top_rate, double other_rate) {
    return std::isfinite(top_rate) && top_rate > 0.0 && top_rate < 1.0 && std::isfinite(other_rate) && other_rate > 0.0 && other_rate <= 1.0 &&
           top_rate + other_rate <= 1.0;
}
static const char* const GOSS_DEBUG_RATES = "top_rate must lie in (0, 1), other_rate in (0, 1], and their sum must be at most 1";

// what is wrong with the tree hook's options (nullptr: nothing): every rule that can be held without the dataset
static const char* hist_tree_options_error(const FrHistTreeOptions& o) {
    if (o.max_depth < 1) return "max_depth must be at least 1";
    if (o.max_leaves == 1) return "max_leaves must be 0 (level-wise) or at least 2";
    for (double x : {o.lambda_l2, o.min_sum_hessian, o.min_split_gain})
        if (!(std::isfinite(x) && x >= 0.0) || (!o.newton && x != 0.0))
            return "lambda_l2, min_sum_hessian and min_split_gain must be finite and at least 0, and 0 without the Newton gain";
    if (o.goss && !goss_debug_rates_ok(o.top_rate, o.other_rate)) return GOSS_DEBUG_RATES;
    if ((o.n_mono != 0 || o.goss) && !o.newton) return "monotone constraints and GOSS need the Newton gain";
    if (o.symmetric && (o.max_leaves != 0 || o.n_mono != 0 || o.goss))
        return "symmetric trees are grown level-wise (max_leaves = 0), without monotone constraints or GOSS";
    for (double x : {o.lambda_l1, o.max_delta_step, o.path_smooth})
        if (!(std::isfinite(x) && x >= 0.0) || (!o.newton && x != 0.0))
            return "lambda_l1, max_delta_step and path_smooth must be finite and at least 0, and 0 without the Newton gain";
    if (o.symmetric && o.path_smooth != 0.0) return "symmetric trees take no path_smooth";
    if (!fr::quant_bits_ok(o.quant_bits)) return "quant_bits must be 0 (off) or between 2 and 8";
    if (o.quant_bits != 0 && (!o.newton || o.n_mono != 0 || o.lambda_l1 != 0.0 || o.max_delta_step != 0.0 || o.path_smooth != 0.0))
        return "quantised gradients need the Newton gain, and take no monotone constraints, lambda_l1, max_delta_step or path_smooth";
    return nullptr;
}

// One tree of the histogram grower (DESIGN.md section 11) for lambda / weight by instance id, under the options
// include/fastrank.h describes; *clamped_leaves_out (may be NULL): the leaves a monotone bound moved.
const CResult* fr_debug_hist_tree(const CDataset* dataset, const FrHistTreeOptions* opt, const double* lambda, const double* weight, size_t len,
                                  uint32_t* clamped_leaves_out) {
    return c_call<CModel>([&]() {
        const std::string who = "fr_debug_hist_tree";
        if (!opt) fr::fail_str("NULL pointer: tree options");
        const FrHistTreeOptions& o = *opt;
        if (const char* wrong = hist_tree_options_error(o)) fr::fail_str(who + ": " + wrong);
        if (clamped_leaves_out) *clamped_leaves_out = 0;
        const CDataset& ds = require_dataset(dataset);
        if (!lambda || !weight) fr::fail_str("NULL pointer: gradient inputs");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        const HistDebugInput in(view, o.queries, o.n_queries);
        const std::vector<uint32_t>& feats = in.feats;
        fr::HistGrowOptions grow{o.split_candidates, o.max_depth, o.min_leaf_support, fr::HistNewton(), o.max_leaves, {}, o.symmetric != 0};
        if (o.newton) grow.newton = {true, o.lambda_l2, o.min_sum_hessian, o.min_split_gain};
        grow.reg = {o.lambda_l1, o.max_delta_step, o.path_smooth};
        grow.quant_bits = o.quant_bits;
        const std::vector<uint32_t> sel = o.features ? hist_debug_selection(who, feats, o.features, o.n_features) : std::vector<uint32_t>();
        if (o.n_mono != 0) {
            if (!o.mono_features || !o.mono_signs) fr::fail_str("NULL pointer: monotone constraints");
            grow.monotone.assign(feats.size(), 0);
            for (size_t i = 0; i < o.n_mono; i++) {
                const auto it = std::lower_bound(feats.begin(), feats.end(), o.mono_features[i]);
                if (it == feats.end() || *it != o.mono_features[i]) fr::fail_str(who + ": feature " + std::to_string(o.mono_features[i]) + " is not in the view");
                if (o.mono_signs[i] < -1 || o.mono_signs[i] > 1) fr::fail_str(who + ": a monotone sign must be -1, 0 or 1");
                grow.monotone[(size_t)(it - feats.begin())] = (int)o.mono_signs[i];
            }
        }
        const std::string too_short = who + ": the gradient arrays are shorter than the largest " + (in.sampled ? "sampled " : "") + "instance id";
        const std::vector<double> lam = in.gather(lambda, len, too_short), wt = in.gather(weight, len, too_short);
        const fr::HistGoss goss{o.top_rate, o.other_rate, fr::GossKeys::of_tree(o.seed, o.tree)};
        HistDebugGrower grower(view, in, grow, o.features ? &sel : nullptr);
        return new_model([&] {
            fr::Model tree;
            tree.kind = fr::Model::DecisionTree;
            fr::HistTreeReport rep;
            tree.tree = grower.g.grow(lam.data(), wt.data(), o.goss ? &goss : nullptr, &rep,
                                    o.quant_bits != 0 ? fr::QuantKeys::of_tree(o.quant_seed, o.quant_tree) : 0);
            if (clamped_leaves_out) *clamped_leaves_out = rep.clamped_leaves;
            return tree;
        });
    });
}

// lambdamart_reg.hpp's output and term of one integer pair, without a device
const void* fr_debug_hist_reg_term(int64_t q, int64_t w, uint32_t n, int32_t s_l, int32_t s_w, double lambda_l1, double lambda_l2,
                                   double max_delta_step, double path_smooth, int32_t has_parent, double parent, double lo, double hi, double* v_out,
                                   double* term_out) {
    return status_call([&]() {
        if (!v_out || !term_out) fr::fail_str("NULL pointer: fr_debug_hist_reg_term");
        const fr::HistReg reg{lambda_l1, max_delta_step, path_smooth};
        const fr::RegSide s = fr::reg_side((long long)q, (long long)w, n, s_l, s_w, lambda_l2, reg, has_parent ? &parent : nullptr, lo, hi);
        *v_out = s.v, *term_out = s.term;
    });
}

// The GOSS selection on its own: lambda[len] by instance id; queries[n_queries] (NULL: all) = the tree's query sample, whose
// instances are the list L.  list_out / top_out[cap] (cap >= the view's instances): the GOSS list as indices into the view's
// full instance list, ascending, and per entry whether it is in the top set; *n_g_out: its length; *tau_out: the n_top-th
// largest key.
const void* fr_debug_goss_select(const CDataset* dataset, const double* lambda, size_t len, double top_rate, double other_rate, uint64_t seed,
                                 uint32_t tree, const uint32_t* queries, size_t n_queries, uint32_t* list_out, uint8_t* top_out, size_t cap,
                                 uint32_t* n_g_out, uint64_t* tau_out) {
    return status_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        if (!lambda || !list_out || !top_out || !n_g_out || !tau_out) fr::fail_str("NULL pointer: fr_debug_goss_select");
        if (!goss_debug_rates_ok(top_rate, other_rate)) fr::fail_str(std::string("fr_debug_goss_select: ") + GOSS_DEBUG_RATES);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        const HistDebugInput in(view, queries, n_queries);
        if (cap < in.ids.size()) fr::fail_str("fr_debug_goss_select: the outputs are shorter than the instance list");
        const std::vector<double> lam = in.gather(lambda, len, "fr_debug_goss_select: the gradient array is shorter than the largest instance id",
                                                  "fr_debug_goss_select: a gradient is not finite");
        frdev::DeviceDataset& dev = view.device();
        const HistDebugGrower grower(view, in, HIST_DEBUG_SMALLEST);
        const fr::GossPlan plan = fr::goss_plan(in.n_t, top_rate, other_rate);
        std::string err;
        uint32_t n_g = 0;
        if (!dev.hist_goss(lam.data(), plan.n_top, plan.p, plan.amp, fr::GossKeys::of_tree(seed, tree), &n_g, tau_out, &err)) fr::fail_str(err);
        if (!dev.hist_goss_download(list_out, top_out, n_g, &err)) fr::fail_str(err);
        *n_g_out = n_g;
    });
}

// One batch of random-forest trees grown by the trainer's own grow_batch with every level recorded (include/fastrank.h;
// DESIGN.md section 5.6).  out == NULL: grow, keep the record, return its JSON header; else hand the kept record's bytes over.
static std::mutex g_rf_levels_mu;
static std::vector<unsigned char> g_rf_levels_blob;
const void* fr_debug_rf_levels(const CDataset* dataset, const uint32_t* root_off, size_t n_trees, const uint32_t* root_ids, const uint32_t* feats,
                               uint32_t nf, uint32_t split_candidates, int32_t split_method, uint32_t min_leaf_support, uint32_t max_depth, void* out,
                               size_t out_bytes) {
    return json_call([&]() {
        const std::string who = "fr_debug_rf_levels";
        if (out) {
            std::lock_guard<std::mutex> lk(g_rf_levels_mu);
            if (out_bytes != g_rf_levels_blob.size())
                fr::fail_str(who + ": the record holds " + std::to_string(g_rf_levels_blob.size()) + " bytes, the buffer " + std::to_string(out_bytes));
            if (out_bytes) std::memcpy(out, g_rf_levels_blob.data(), out_bytes);
            std::vector<unsigned char>().swap(g_rf_levels_blob);
            return frjson::dump(Value::object());
        }
        const CDataset& ds = require_dataset(dataset);
        if (!root_off || !root_ids || !feats) fr::fail_str("NULL pointer: " + who);
        if (n_trees == 0 || nf == 0 || split_method < 0 || split_method > 3) fr::fail_str(who + ": at least one tree and one feature, split_method 0..3");
        for (size_t t = 0; t < n_trees; t++)
            if (root_off[t + 1] < root_off[t]) fr::fail_str(who + ": root_off must not decrease");
        if (root_off[0] != 0) fr::fail_str(who + ": root_off must start at 0");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        const std::vector<uint32_t> off(root_off, root_off + n_trees + 1), ids(root_ids, root_ids + root_off[n_trees]), fl(feats, feats + n_trees * nf);
        for (uint32_t f : fl)
            if (std::find(ds.view->features.begin(), ds.view->features.end(), f) == ds.view->features.end())
                fr::fail_str(who + ": feature " + std::to_string(f) + " is not in the view");
        {
            std::vector<char> in_view(ds.view->core->n, 0);
            for (uint32_t id : ds.view->instances)
                if (id < in_view.size()) in_view[id] = 1;
            for (uint32_t id : ids)
                if (id >= in_view.size() || !in_view[id]) fr::fail_str(who + ": instance " + std::to_string(id) + " is not in the view");
        }
        fr::RFParams p;
        p.quiet = true;
        p.num_trees = (uint32_t)n_trees;
        p.split_method = split_method;
        p.min_leaf_support = min_leaf_support;
        p.split_candidates = split_candidates;
        p.max_depth = max_depth;
        fr::RFTrainer trainer(ds.view, fr::Evaluator(), p);
        fr::RFRecorder rec;
        const fr::Model forest = trainer.grow_recorded(off, ids, nf, fl, rec);
        std::vector<unsigned char> blob;
        Value sections = Value::array();
        auto put = [&](size_t level, const char* name, const void* data, size_t bytes) {
            Value s = Value::object();
            s.set("level", Value::uint(level));
            s.set("name", Value::string(name));
            s.set("offset", Value::uint(blob.size()));
            s.set("bytes", Value::uint(bytes));
            sections.push(s);
            const unsigned char* b = static_cast<const unsigned char*>(data);
            if (bytes) blob.insert(blob.end(), b, b + bytes);
        };
        Value levels = Value::array();
        for (size_t i = 0; i < rec.levels.size(); i++) {
            const fr::RFLevelRecord& lv = rec.levels[i];
            Value l = Value::object();
            l.set("A", Value::uint(lv.active.size()));
            l.set("items", Value::uint(lv.svals.size()));
            l.set("children_from", Value::string(lv.children_from_cands ? "candidates" : "rf_childsum_kernel"));
            levels.push(l);
            put(i, "active", lv.active.data(), lv.active.size() * sizeof(lv.active[0]));
            put(i, "depth", lv.depth.data(), lv.depth.size() * 4);
            put(i, "label_minmax", lv.label_minmax.data(), lv.label_minmax.size() * 4);
            put(i, "cands", lv.cands.data(), lv.cands.size() * sizeof(lv.cands[0]));
            put(i, "svals", lv.svals.data(), lv.svals.size() * 4);
            put(i, "sv", lv.sv.data(), lv.sv.size() * 4);
            put(i, "sg", lv.sg.data(), lv.sg.size() * 4);
            put(i, "splits", lv.splits.data(), lv.splits.size() * sizeof(lv.splits[0]));
            put(i, "child_out", lv.child_out.data(), lv.child_out.size() * 8);
        }
        put(rec.levels.size(), "root_out", rec.root_out.data(), rec.root_out.size() * 8);
        Value o = Value::object();
        o.set("cand_bytes", Value::uint(sizeof(frdev::DeviceDataset::RfCand)));
        o.set("levels", levels);
        o.set("sections", sections);
        o.set("bytes", Value::uint(blob.size()));
        Value trees = Value::array();
        for (const fr::Model& m : forest.members) trees.push(fr::model_to_json(m));
        o.set("trees", trees);
        {
            std::lock_guard<std::mutex> blk(g_rf_levels_mu);
            g_rf_levels_blob.swap(blob);
        }
        return frjson::dump(o);
    });
}

// The fixed-point step and the quantised gradients of one tree on their own (DESIGN.md section 11, "Quantised gradients").
const void* fr_debug_hist_quantise(const CDataset* dataset, const double* lambda, const double* weight, size_t len, uint32_t bits, uint64_t seed,
                                   uint32_t tree, const uint32_t* queries, size_t n_queries, int32_t goss, double top_rate, double other_rate,
                                   uint64_t goss_seed, uint32_t goss_tree, int32_t* q_out, uint32_t* w_out, size_t cap, uint32_t* n_out,
                                   int32_t* numbers_out) {
    return status_call([&]() {
        const std::string who = "fr_debug_hist_quantise";
        const CDataset& ds = require_dataset(dataset);
        if (!lambda || !weight || !q_out || !w_out || !n_out || !numbers_out) fr::fail_str("NULL pointer: " + who);
        if (bits < fr::QUANT_MIN_BITS || bits > fr::QUANT_MAX_BITS) fr::fail_str(who + ": bits must be between 2 and 8");
        if (goss && !goss_debug_rates_ok(top_rate, other_rate)) fr::fail_str(who + ": " + GOSS_DEBUG_RATES);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        const HistDebugInput in(view, queries, n_queries);
        if (cap < in.ids.size()) fr::fail_str(who + ": the outputs are shorter than the instance list");
        const std::string too_short = who + ": the gradient arrays are shorter than the largest instance id";
        const std::vector<double> lam = in.gather(lambda, len, too_short), wt = in.gather(weight, len, too_short);
        frdev::DeviceDataset& dev = view.device();
        const HistDebugGrower grower(view, in, HIST_DEBUG_SMALLEST);
        std::string err;
        uint32_t n = (uint32_t)in.n_t;
        if (goss) {
            const fr::GossPlan plan = fr::goss_plan(in.n_t, top_rate, other_rate);
            if (!dev.hist_goss(lam.data(), plan.n_top, plan.p, plan.amp, fr::GossKeys::of_tree(goss_seed, goss_tree), &n, nullptr, &err)) fr::fail_str(err);
        }
        int s_l = 0, s_w = 0, d = 0, d_w = 0;
        bool all_zero = false;
        if (!dev.hist_quantise(lam.data(), wt.data(), &s_l, &s_w, &all_zero, &err)) fr::fail_str(err);
        if (all_zero) fr::fail_str(who + ": every lambda is zero (the tree is one leaf, nothing is quantised)");
        if (!dev.hist_quantq(bits, fr::QuantKeys::of_tree(seed, tree), &d, &d_w, &err)) fr::fail_str(err);
        if (!dev.hist_quantq_download(q_out, w_out, n, &err)) fr::fail_str(err);
        *n_out = n;
        const int32_t numbers[6] = {s_l, s_w, s_l - d, s_w - d_w, d, d_w};
        std::copy(numbers, numbers + 6, numbers_out);
    });
}

// The root's histogram of one tree (count, sum Q, sum W as [features][k]) for lambda / weight by instance id: bits == 0 by the
// Newton build over Q / W, else by the packed build over the quantised values of tree `tree` of `seed`.
const void* fr_debug_hist_root_histogram(const CDataset* dataset, const double* lambda, const double* weight, size_t len, uint32_t split_candidates,
                                         uint32_t bits, uint64_t seed, uint32_t tree, const uint32_t* features, size_t n_features,
                                         uint32_t* count_out, int64_t* sum_out, int64_t* wsum_out, size_t cells) {
    return status_call([&]() {
        const std::string who = "fr_debug_hist_root_histogram";
        const CDataset& ds = require_dataset(dataset);
        if (!lambda || !weight || !count_out || !sum_out || !wsum_out) fr::fail_str("NULL pointer: " + who);
        if (!fr::quant_bits_ok(bits)) fr::fail_str(who + ": bits must be 0 or between 2 and 8");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        const HistDebugInput in(view, nullptr, 0);
        const std::vector<uint32_t>& feats = in.feats;
        const std::vector<uint32_t> sel = features ? hist_debug_selection(who, feats, features, n_features) : std::vector<uint32_t>();
        const size_t Ft = features ? sel.size() : feats.size();
        if (cells != Ft * (size_t)split_candidates) fr::fail_str(who + ": the outputs must hold features x split_candidates cells");
        const std::string too_short = who + ": the gradient arrays are shorter than the largest instance id";
        const std::vector<double> lam = in.gather(lambda, len, too_short), wt = in.gather(weight, len, too_short);
        frdev::DeviceDataset& dev = view.device();
        const HistDebugGrower grower(view, in, {split_candidates, 1u, 1u, fr::HistNewton{true, 0.0, 0.0, 0.0}, 0u, {}}, features ? &sel : nullptr);
        std::string err;
        int s_l = 0, s_w = 0, d = 0, d_w = 0;
        bool all_zero = false;
        if (!dev.hist_quantise(lam.data(), wt.data(), &s_l, &s_w, &all_zero, &err)) fr::fail_str(err);
        if (all_zero) fr::fail_str(who + ": every lambda is zero (no fixed-point values are made)");
        if (bits != 0 && !dev.hist_quantq(bits, fr::QuantKeys::of_tree(seed, tree), &d, &d_w, &err)) fr::fail_str(err);
        if (!dev.hist_root(true, &err)) fr::fail_str(err);
        static_assert(sizeof(long long) == sizeof(int64_t), "the histograms' sums are 64-bit");
        if (!dev.hist_root_download(count_out, reinterpret_cast<long long*>(sum_out), reinterpret_cast<long long*>(wsum_out), cells, &err)) fr::fail_str(err);
    });
}

}  // extern "C"
