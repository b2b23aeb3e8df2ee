// capi.cpp: the neural LambdaRank trainer's host loop (DESIGN.md section 19; neural_lambda.hpp holds its parameters,
// initialiser, Adam step and statistics) and its two test hooks.  Every stage runs on the view's primary device: a request
// that names several devices gets the single-device model, as LambdaMART's does.
namespace {

fr::Model train_neural_lambdarank(const std::shared_ptr<fr::DatasetView>& view, const ParsedRequest& rq) {
    const auto tnow = [] { return std::chrono::steady_clock::now(); };
    const auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double>(b - a).count();
    };
    const auto t0 = tnow();
    const fr::NeuralLambdaRankParams& p = rq.nl;
    fr::NeuralLambdaRankStats st;
    st.request = p;
    // under objective = map / mrr the AP / RR evaluator takes over every role of the request's measure (which was checked)
    const char* objective = p.objective_measure();
    const fr::Evaluator ev = fr::make_evaluator(*view, objective ? std::string(objective) : rq.measure, rq.has_qrel ? &rq.qrel : nullptr);
    if (ev.measure != p.objective_evaluator())
        fr::fail_str(std::string("NeuralLambdaRank: the evaluator does not belong to the objective `") + fr::LambdaMARTParams::objective_name(p.objective) + "`");
    const std::vector<uint32_t> feats = features_ascending(*view);
    if (feats.empty()) fr::fail_str("assertion failed: !features.is_empty()");
    if (view->host_csr().nq == 0) fr::fail_str("assertion failed: !data.queries().is_empty()");
    frdev::DeviceDataset& dev = view->device();
    const size_t d = dev.d(), h = p.hidden, h2 = p.hidden2;
    {
        const std::vector<double>& absmax = dev.column_absmax();
        for (uint32_t f : feats)
            if (f < absmax.size() && !std::isfinite(absmax[f]))
                fr::fail_str("NeuralLambdaRank: feature " + std::to_string(f) + " holds an inf or NaN value (in this dataset, or in the dataset it is a "
                             "query view of); the net is only trained over finite feature values");
    }
    st.features = (uint32_t)feats.size();
    std::string err;
    std::vector<unsigned char> flags;
    fr::Model net = fr::neural_init(p.seed, h, d, feats, &flags, h2);
    const size_t n = flags.size(), nw = h * d;
    std::vector<double> theta = fr::neural_flatten(net), grad(n, 0.0), am(n, 0.0), av(n, 0.0);
    // scores of the net into slot 0, waited for
    auto score = [&]() {
        if (h2 != 0) {
            if (!dev.score_mlp2(fr::mlp2_net_of(net), &err, &st.score_plan)) fr::fail_str(err);
        } else if (!dev.score_mlp(h, d, net.nn_w1.data(), net.nn_b1.data(), net.nn_w2.data(), net.nn_b2, &err, &st.score_plan)) {
            fr::fail_str(err);
        }
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
    st.initial_measure = measure();
    st.t_measure += secs(tb, tnow());
    if (p.trace) st.initial = fr::model_to_json(net);
    if (!p.quiet) printf("-----------------------\n|%7s|%15s|\n-----------------------\n|%7u|%15.6f|\n", "Iter", ev.name.c_str(), 0u, st.initial_measure);
    fr::Model best_net = net;  // the iterate neural_lambda_best names among those so far
    for (uint32_t t = 0; t < p.num_iterations; t++) {
        // (slot 0 holds the scores of the current net: the measure pass of the iteration before left them there)
        ta = tnow();
        if (!dev.lambda_gradients(ev.norms.data(), ev.depth, p.sigma, p.pass(), &err)) fr::fail_str(err);
        if (!frdev::device_synchronize(&err)) fr::fail_str(err);
        tb = tnow();
        st.t_gradient += secs(ta, tb);
        if (h2 != 0) {  // (the record's order is the parameters')
            if (!dev.mlp2_backprop(fr::mlp2_net_of(net), nullptr, nullptr, grad.data(), &err, &st.backprop_plan)) fr::fail_str(err);
        } else if (!dev.mlp_backprop(h, d, net.nn_w1.data(), net.nn_b1.data(), net.nn_w2.data(), nullptr, nullptr, grad.data(), grad.data() + nw,
                                     grad.data() + nw + h, grad.data() + nw + 2 * h, &err, &st.backprop_plan)) {
            fr::fail_str(err);
        }
        ta = tnow();
        st.t_backprop += secs(tb, ta);
        fr::adam_step(theta.data(), grad.data(), am.data(), av.data(), n, flags.data(), t + 1, p.learning_rate, p.lambda_l2);
        fr::neural_unflatten(theta, &net);
        tb = tnow();
        st.t_adam += secs(ta, tb);
        score();
        ta = tnow();
        st.t_score += secs(tb, ta);
        const double mean = measure();
        st.t_measure += secs(ta, tnow());
        st.train_measure.push_back(mean);
        if (p.trace) st.iterates.push(fr::model_to_json(net));
        if (fr::neural_lambda_best(st.initial_measure, st.train_measure) == t + 1) best_net = net;
        if (!p.quiet) {
            printf("|%7u|%15.6f|\n", t + 1, mean);
            fflush(stdout);
        }
    }
    if (!p.quiet) printf("-----------------------\n");
    st.iterations = p.num_iterations;
    st.best_iteration = fr::neural_lambda_best(st.initial_measure, st.train_measure);
    st.seconds = secs(t0, tnow());
    fr::TrainStats ts;
    ts.devices = 1;
    ts.path = "neural_lambdarank";
    ts.seconds = st.seconds;
    ts.restarts = st.iterations;
    set_last_stats(ts);
    std::lock_guard<std::mutex> lk(g_stats_mu);
    g_last_neural_lambdarank = st.to_json();
    return best_net;
}

}  // namespace

extern "C" {

// Back-propagation through `model` (a NeuralNet) on an uploaded lambda by instance id (len entries; an id the view holds must
// be below len), queries[n_queries] = indices of the view's queries to visit (NULL: all).  Positions that hold no document of
// the view are uploaded as NaN.  g_w1[h * d] row-major over the dataset's d columns, g_b1[h], g_w2[h], g_b2[1].  Returns the
// plan as JSON with "h" and "d"; with the outputs NULL nothing runs and the reply holds only the sizes.
const void* fr_debug_mlp_gradients(const CDataset* dataset, const CModel* model, const double* lambda, size_t len, const uint32_t* queries,
                                   size_t n_queries, double* g_w1, double* g_b1, double* g_w2, double* g_b2) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        const CModel& cm = require_model(model);
        if (cm.actual.kind != fr::Model::NeuralNet) fr::fail_str("fr_debug_mlp_gradients: the model must be a NeuralNet");
        const fr::Model& net = cm.actual;
        // nn_w2 of a two-layer net holds h2 numbers, not h: the one-layer launcher must not see it
        if (net.nn_hidden2() != 0)
            fr::fail_str("fr_debug_mlp_gradients: the model has hidden2_weights; its gradients come from fr_debug_mlp2_gradients");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) fr::fail_str("fr_debug_mlp_gradients: the dataset holds no instance");
        frdev::DeviceDataset& dev = view.device();
        Value o = Value::object();
        o.set("h", Value::uint(net.nn_b1.size()));
        o.set("d", Value::uint(dev.d()));
        if (!g_w1 && !g_b1 && !g_w2 && !g_b2) return frjson::dump(o);  // the size question: nothing runs
        if (!lambda || !g_w1 || !g_b1 || !g_w2 || !g_b2) fr::fail_str("NULL pointer: fr_debug_mlp_gradients");
        std::vector<unsigned char> flags;
        if (queries) flags = debug_query_flags(queries, n_queries, view.host_csr().nq);
        size_t np = 0;
        const uint32_t* instance_at = dev.position_instances(&np);
        std::vector<double> lam(np, std::numeric_limits<double>::quiet_NaN());
        for (size_t pos = 0; pos < np; pos++) {
            const uint32_t id = instance_at[pos];
            if (id == 0xFFFFFFFFu) continue;
            if (id >= len) fr::fail_str("fr_debug_mlp_gradients: the gradient array is shorter than the largest instance id");
            lam[pos] = lambda[id];
        }
        std::string err;
        frdev::DeviceDataset::MlpPlan plan;
        if (!dev.mlp_backprop(net.nn_b1.size(), net.nn_cols, net.nn_w1.data(), net.nn_b1.data(), net.nn_w2.data(), lam.data(),
                              queries ? flags.data() : nullptr, g_w1, g_b1, g_w2, g_b2, &err, &plan))
            fr::fail_str(err);
        const Value pj = fr::mlp_plan_json(plan);
        for (const auto& kv : pj.obj) o.set(kv.first.c_str(), kv.second);
        return frjson::dump(o);
    });
}

// fr_debug_mlp_gradients for a NeuralNet with a second hidden layer: the six arrays under the model's key names, g_w1[h * d]
// row-major over the dataset's d columns, g_b1[h], g_w2[h2 * h] row-major, g_c[h2], g_w3[h2], g_bout[1].  Returns the plan as
// JSON with "h", "h2" and "d"; with the outputs NULL nothing runs and the reply holds only the sizes.
const void* fr_debug_mlp2_gradients(const CDataset* dataset, const CModel* model, const double* lambda, size_t len, const uint32_t* queries,
                                    size_t n_queries, double* g_w1, double* g_b1, double* g_w2, double* g_c, double* g_w3, double* g_bout) {
    return json_call([&]() {
        const CDataset& ds = require_dataset(dataset);
        const CModel& cm = require_model(model);
        const fr::Model& net = cm.actual;
        if (net.kind != fr::Model::NeuralNet || net.nn_hidden2() == 0)
            fr::fail_str("fr_debug_mlp2_gradients: the model must be a NeuralNet with hidden2_weights");
        std::lock_guard<std::mutex> lk(api_mu_of(ds));
        fr::DatasetView& view = *ds.view;
        if (view.instances.empty()) fr::fail_str("fr_debug_mlp2_gradients: the dataset holds no instance");
        frdev::DeviceDataset& dev = view.device();
        const size_t h = net.nn_b1.size(), h2 = net.nn_hidden2(), d = dev.d();
        Value o = Value::object();
        o.set("h", Value::uint(h));
        o.set("h2", Value::uint(h2));
        o.set("d", Value::uint(d));
        double* const outs[] = {g_w1, g_b1, g_w2, g_c, g_w3, g_bout};
        const size_t sizes[] = {h * d, h, h2 * h, h2, h2, 1};
        size_t given = 0;
        for (double* q : outs) given += q != nullptr;
        if (given == 0) return frjson::dump(o);  // the size question: nothing runs
        if (!lambda || given != 6) fr::fail_str("NULL pointer: fr_debug_mlp2_gradients");
        std::vector<unsigned char> flags;
        if (queries) flags = debug_query_flags(queries, n_queries, view.host_csr().nq);
        size_t np = 0;
        const uint32_t* instance_at = dev.position_instances(&np);
        std::vector<double> lam(np, std::numeric_limits<double>::quiet_NaN());
        for (size_t pos = 0; pos < np; pos++) {
            const uint32_t id = instance_at[pos];
            if (id == 0xFFFFFFFFu) continue;
            if (id >= len) fr::fail_str("fr_debug_mlp2_gradients: the gradient array is shorter than the largest instance id");
            lam[pos] = lambda[id];
        }
        std::string err;
        frdev::DeviceDataset::MlpPlan plan;
        std::vector<double> grad(h * d + h + h2 * h + 2 * h2 + 1);
        if (!dev.mlp2_backprop(fr::mlp2_net_of(net), lam.data(), queries ? flags.data() : nullptr, grad.data(), &err, &plan)) fr::fail_str(err);
        const double* at = grad.data();
        for (size_t k = 0; k < 6; at += sizes[k], k++) std::copy(at, at + sizes[k], outs[k]);
        const Value pj = fr::mlp_plan_json(plan);
        for (const auto& kv : pj.obj) o.set(kv.first.c_str(), kv.second);
        return frjson::dump(o);
    });
}

// The trainer's Adam step alone (neural_lambda.hpp: adam_step; no device), in place on theta / m / v [n]; decays[n] (NULL: no
// parameter): 1 where lambda_l2 applies; t: the 1-based step.
const void* fr_debug_adam_step(double* theta, const double* grad, double* m, double* v, size_t n, const unsigned char* decays, uint32_t t,
                               double learning_rate, double lambda_l2) {
    return status_call([&]() {
        if (n && (!theta || !grad || !m || !v)) fr::fail_str("NULL pointer: fr_debug_adam_step");
        if (t < 1) fr::fail_str("fr_debug_adam_step: steps are numbered from 1");
        std::vector<unsigned char> flags(n, fr::ADAM_UPDATED);
        for (size_t c = 0; decays && c < n; c++)
            if (decays[c]) flags[c] |= fr::ADAM_DECAYS;
        fr::adam_step(theta, grad, m, v, n, flags.data(), t, learning_rate, lambda_l2);
    });
}

}  // extern "C"
