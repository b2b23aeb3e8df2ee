// capi.cpp: the linear LambdaRank trainer's host loop (DESIGN.md section 18; linear_lambda.hpp holds its parameters, solver and
// statistics) and its two test hooks.  Every stage runs on the view's primary device: a request that names several devices
// gets the single-device model, as LambdaMART's does.
namespace {

fr::Model train_linear_lambdarank(const std::shared_ptr<fr::DatasetView>& view, const ParsedRequest& rq) {
    const auto tnow = [] { return std::chrono::steady_clock::now(); };
    const auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double>(b - a).count();
    };
    const auto t0 = tnow();
    const fr::LinearLambdaRankParams& p = rq.ll;
    fr::LinearLambdaRankStats st;
    st.request = p;
    // under objective = map / mrr the AP / RR evaluator takes over every role of the request's measure (which was checked)
    const char* objective = p.objective_measure();
    const fr::Evaluator ev = fr::make_evaluator(*view, objective ? std::string(objective) : rq.measure, rq.has_qrel ? &rq.qrel : nullptr);
    if (ev.measure != p.objective_evaluator())
        fr::fail_str(std::string("LinearLambdaRank: the evaluator does not belong to the objective `") + fr::LambdaMARTParams::objective_name(p.objective) + "`");
    const std::vector<uint32_t> feats = features_ascending(*view);
    if (feats.empty()) fr::fail_str("assertion failed: !features.is_empty()");
    if (view->host_csr().nq == 0) fr::fail_str("assertion failed: !data.queries().is_empty()");
    frdev::DeviceDataset& dev = view->device();
    const size_t d = dev.d(), F = feats.size();
    {
        const std::vector<double>& absmax = dev.column_absmax();
        for (uint32_t f : feats)
            if (f < absmax.size() && !std::isfinite(absmax[f]))
                fr::fail_str("LinearLambdaRank: feature " + std::to_string(f) + " holds an inf or NaN value (in this dataset, or in the dataset it is a "
                             "query view of); the Newton matrix is only formed over finite feature values");
    }
    st.features = (uint32_t)F;
    std::string err;
    std::vector<double> w(d, 0.0), H(d * d), g(d), Hs(F * F), gs(F), delta(F);
    // scores of Linear(w) into slot 0, waited for
    auto score = [&]() {
        if (!dev.score_linear(1, w.data(), &err)) fr::fail_str(err);
        if (!frdev::device_synchronize(&err)) fr::fail_str(err);
    };
    // the measure's mean of the scores in slot 0
    auto measure = [&]() {
        double mean = 0.0;
        evaluate_scores(dev, ev, 1);
        if (!dev.reduce_means(1, &mean, &err)) fr::fail_str(err);
        return mean;
    };
    auto ta = tnow();
    score();
    auto tb = tnow();
    st.t_score += secs(ta, tb);
    st.zero_measure = measure();
    st.t_measure += secs(tb, tnow());
    if (!p.quiet) printf("-----------------------\n|%7s|%15s|\n-----------------------\n|%7u|%15.6f|\n", "Iter", ev.name.c_str(), 0u, st.zero_measure);
    for (uint32_t t = 0; t < p.num_iterations; t++) {
        // (slot 0 holds the scores of Linear(w^t): the measure pass of the iteration before left them there)
        ta = tnow();
        if (!dev.lambda_gradients(ev.norms.data(), ev.depth, p.sigma, p.pass(), &err)) fr::fail_str(err);
        if (!frdev::device_synchronize(&err)) fr::fail_str(err);
        tb = tnow();
        st.t_gradient += secs(ta, tb);
        if (!dev.weighted_gram(nullptr, nullptr, nullptr, H.data(), g.data(), &err, &st.plan)) fr::fail_str(err);
        ta = tnow();
        st.t_gram += secs(tb, ta);
        // the view's features, ascending: the others' weights stay 0
        for (size_t i = 0; i < F; i++) {
            gs[i] = g[feats[i]];
            for (size_t j = 0; j < F; j++) Hs[i * F + j] = H[(size_t)feats[i] * d + feats[j]];
        }
        double pivot = 0.0;
        const int bad = fr::newton_step(Hs.data(), gs.data(), F, p.lambda_l2, delta.data(), &pivot);
        if (bad >= 0)
            fr::fail_str(fr::newton_pivot_message("`" + view->core->feature_name(feats[(size_t)bad]) + "` (iteration " + std::to_string(t) + ")", pivot, p.lambda_l2));
        for (size_t i = 0; i < F; i++) {
            const double step = p.learning_rate * delta[i];
            w[feats[i]] = w[feats[i]] + step;
        }
        tb = tnow();
        st.t_solve += secs(ta, tb);
        score();
        ta = tnow();
        st.t_score += secs(tb, ta);
        const double mean = measure();
        st.t_measure += secs(ta, tnow());
        st.train_measure.push_back(mean);
        st.weights.push_back(w);
        if (!p.quiet) {
            printf("|%7u|%15.6f|\n", t + 1, mean);
            fflush(stdout);
        }
    }
    if (!p.quiet) printf("-----------------------\n");
    st.iterations = p.num_iterations;
    st.best_iteration = fr::linear_lambda_best(st.zero_measure, st.train_measure);
    fr::Model m;
    m.kind = fr::Model::Linear;
    m.weights = st.weights[st.best_iteration - 1];
    st.seconds = secs(t0, tnow());
    fr::TrainStats ts;
    ts.devices = 1;
    ts.path = "linear_lambdarank";
    ts.seconds = st.seconds;
    ts.restarts = st.iterations;
    set_last_stats(ts);
    std::lock_guard<std::mutex> lk(g_stats_mu);
    g_last_linear_lambdarank = st.to_json();
    return m;
}

}  // namespace

extern "C" {

// The Gram kernel pair on uploaded arrays: lambda / weight by instance id (len entries; an id the view holds must be below
// len), queries[n_queries] = indices of the view's queries to visit (NULL: all).  Positions that hold no document of the view
// are uploaded as NaN.  h_out[d * d] row-major, g_out[d], d = the dataset's columns.  Returns the plan as JSON; with both
// outputs NULL nothing runs and the reply is {"d": the dataset's columns}.
const void* fr_debug_weighted_gram(const CDataset* dataset, const double* lambda, const double* weight, size_t len, const uint32_t* queries,
                                   size_t n_queries, double* h_out, double* g_out, size_t d) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) fr::fail_str("fr_debug_weighted_gram: the dataset holds no instance");
        frdev::DeviceDataset& dev = view.device();
        if (!h_out && !g_out) {  // the size question: nothing runs
            Value o = Value::object();
            o.set("d", Value::uint(dev.d()));
            return frjson::dump(o);
        }
        if (!lambda || !weight || !h_out || !g_out) fr::fail_str("NULL pointer: fr_debug_weighted_gram");
        if (d != dev.d()) fr::fail_str("fr_debug_weighted_gram: the outputs must hold " + std::to_string(dev.d()) + " columns");
        std::vector<unsigned char> flags;
        if (queries) flags = debug_query_flags(queries, n_queries, view.host_csr().nq);
        size_t np = 0;
        const uint32_t* instance_at = dev.position_instances(&np);
        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::vector<double> lam(np, nan), wt(np, nan);
        for (size_t pos = 0; pos < np; pos++) {
            const uint32_t id = instance_at[pos];
            if (id == 0xFFFFFFFFu) continue;
            if (id >= len) fr::fail_str("fr_debug_weighted_gram: the gradient arrays are shorter than the largest instance id");
            lam[pos] = lambda[id], wt[pos] = weight[id];
        }
        std::string err;
        frdev::DeviceDataset::GramPlan plan;
        if (!dev.weighted_gram(lam.data(), wt.data(), queries ? flags.data() : nullptr, h_out, g_out, &err, &plan)) fr::fail_str(err);
        Value o = Value::object();
        o.set("passes", Value::uint(plan.passes));
        o.set("workgroups", Value::uint(plan.workgroups));
        o.set("stretch_tiles", Value::uint(plan.stretch));
        o.set("tiles", Value::uint(plan.tiles));
        o.set("slab_bytes", Value::uint(plan.slab_bytes));
        o.set("tile_bytes", Value::uint(plan.tile_bytes));
        return frjson::dump(o);
    });
}

// The trainer's host solver alone (linear_lambda.hpp: newton_step; no device): delta_out[n] of (H + lambda_l2 I) delta = g.
const void* fr_debug_newton_step(const double* h, const double* g, size_t n, double lambda_l2, double* delta_out) {
    return status_call([&]() {
        if (n && (!h || !g || !delta_out)) fr::fail_str("NULL pointer: fr_debug_newton_step");
        double pivot = 0.0;
        const int bad = fr::newton_step(h, g, n, lambda_l2, delta_out, &pivot);
        if (bad >= 0) fr::fail_str(fr::newton_pivot_message(std::to_string(bad), pivot, lambda_l2));
    });
}

}  // extern "C"
