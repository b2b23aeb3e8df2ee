// The neural LambdaRank trainer's host side (host only, no HIP): the request's parameters and their wire
// form, the initialiser, the Adam step, the choice of the returned iterate, the statistics.  The loop that drives the device is
// train_neural_lambda.inc.
//
// Parameters are numbered in wire order over the dataset's d columns: c = j d + i for W1[j][i], h d + j for b1[j],
// h d + h + j for w2[j], h d + 2 h for b2.
//
// Initialiser.  K = mix(seed + 4 GOLDEN) (resample.hpp; 1 .. 3 are boot_key, perm_key, stream_key); u_c = (mix(K + c) >> 11) 2^-53.
// W1[j][i] = fl(fl(fl(2 u_c) - 1) * s1), s1 = sqrt(fl(6 / (F + h))), for the F columns the view holds; w2[j] likewise with
// s2 = sqrt(fl(6 / (h + 1))); every other parameter starts at 0.
//
// Adam ascent step t (1-based), per updated parameter, every product, quotient and sum rounded separately, in this order:
//   g' = decays ? g - fl(lambda_l2 * theta) : g
//   m = fl(0.9 * m) + fl(fl(1 - 0.9) * g')             v = fl(0.999 * v) + fl(fl(1 - 0.999) * fl(g' * g'))
//   mh = m / (1 - 0.9^t)    vh = v / (1 - 0.999^t)     (the powers by t - 1 successive multiplications)
//   theta = theta + fl(fl(learning_rate * mh) / fl(sqrt(vh) + 1e-8))
// W1 and w2 decay, the biases do not; columns the view does not hold are not updated.
//
// With `hidden2` (a second hidden layer of h2 units; DESIGN.md section 19, "Two hidden layers") the numbering goes on after b1:
// h d + h + k h + j for W2[k][j], then h2 numbers c[k], h2 numbers w3[k] (the model's output_weights), then b_out.  W1 is drawn
// as above, bit for bit; W2[k][j] = fl(fl(fl(2 u_c) - 1) * s2) with s2 = sqrt(fl(6 / (h + h2))), w3[k] likewise with
// s3 = sqrt(fl(6 / (h2 + 1))), each under its own number c.  W1, W2 and w3 decay.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "lambdamart.hpp"
#include "resample.hpp"

namespace fr {

struct NeuralLambdaRankParams {
    // (hidden, num_iterations, learning_rate: chosen by training NDCG on the bundled example)
    uint32_t hidden = 64;
    uint32_t num_iterations = 100;
    double learning_rate = 0.03;
    double lambda_l2 = 0.0;
    double sigma = 1.0;
    uint64_t seed = 0;
    bool quiet = false;
    // the gradient pass's keys, LambdaMART's, and the trace switch (optional, not written at their defaults)
    int objective = frdev::M_NDCG;
    uint32_t truncation_level = 0;
    bool lambda_norm = false;
    bool trace = false;
    uint32_t hidden2 = 0;  // units of a second hidden layer (0: none; optional, written only when it is set)

    bool xendcg() const { return objective == frdev::LM_OBJECTIVE_XENDCG; }
    bool approxndcg() const { return objective == frdev::LM_OBJECTIVE_APPROXNDCG; }
    int objective_evaluator() const { return xendcg() || approxndcg() ? (int)frdev::M_NDCG : objective; }
    const char* objective_measure() const { return objective == frdev::M_AP ? "ap" : objective == frdev::M_RR ? "rr" : nullptr; }
    frdev::DeviceDataset::LambdaPass pass() const { return {nullptr, false, truncation_level, lambda_norm, objective, 0}; }

    static NeuralLambdaRankParams from_json(const Value& v) {
        if (!v.is_object()) fail_raw("Error(\"invalid type: expected struct NeuralLambdaRankParams\", line: 0, column: 0)");
        const std::pair<const char*, const char*> out_of_scope[] = {
            {"validation_queries", "held-out queries are not supported by NeuralLambdaRank (hold them out of the dataset with a query sample)"},
            {"early_stopping_rounds", "held-out queries are not supported by NeuralLambdaRank (the best training iteration is returned)"},
            {"init_model", "init_model is not supported by NeuralLambdaRank (training starts from the seeded initial net)"},
            {"valid", "a validation dataset is not supported by NeuralLambdaRank"},
            {"validation_dataset", "a validation dataset is not supported by NeuralLambdaRank"}};
        for (const auto& kv : out_of_scope)
            if (v.find(kv.first)) LambdaMARTParams::invalid(kv.second);
        NeuralLambdaRankParams p;
        p.hidden = json_u32(json_field(v, "hidden"), "hidden");
        p.num_iterations = json_u32(json_field(v, "num_iterations"), "num_iterations");
        p.learning_rate = json_f64(json_field(v, "learning_rate"), "learning_rate");
        p.lambda_l2 = json_f64(json_field(v, "lambda_l2"), "lambda_l2");
        p.sigma = json_f64(json_field(v, "sigma"), "sigma");
        p.seed = json_u64(json_field(v, "seed"), "seed");
        p.quiet = json_bool(json_field(v, "quiet"), "quiet");
        if (const Value* g = v.find("objective")) p.objective = LambdaMARTParams::objective_from_json(*g);
        if (const Value* r = v.find("truncation_level")) p.truncation_level = json_u32(*r, "truncation_level");
        if (const Value* r = v.find("lambda_norm")) p.lambda_norm = json_bool(*r, "lambda_norm");
        if (const Value* r = v.find("trace")) p.trace = json_bool(*r, "trace");
        const Value* h2 = v.find("hidden2");
        if (h2) p.hidden2 = json_u32(*h2, "hidden2");
        for (const auto& kv : v.obj) {
            static const char* known[] = {"hidden", "num_iterations", "learning_rate", "lambda_l2", "sigma", "seed", "quiet", "objective",
                                          "truncation_level", "lambda_norm", "trace", "hidden2"};
            bool ok = false;
            for (const char* k : known) ok = ok || kv.first == k;
            if (!ok) fail_raw("Error(\"unknown field `" + kv.first + "` of NeuralLambdaRankParams\", line: 0, column: 0)");
        }
        if (p.hidden < 1 || p.hidden > 1024) LambdaMARTParams::invalid("hidden must be between 1 and 1024");
        if (h2 && (p.hidden2 < 1 || p.hidden2 > 64)) LambdaMARTParams::invalid("hidden2 must be between 1 and 64");
        if (p.num_iterations < 1) LambdaMARTParams::invalid("num_iterations must be at least 1");
        if (!(std::isfinite(p.learning_rate) && p.learning_rate > 0.0)) LambdaMARTParams::invalid("learning_rate must be finite and greater than 0");
        if (!(std::isfinite(p.lambda_l2) && p.lambda_l2 >= 0.0)) LambdaMARTParams::invalid("lambda_l2 must be finite and at least 0");
        if (!(std::isfinite(p.sigma) && p.sigma > 0.0)) LambdaMARTParams::invalid("sigma must be finite and greater than 0");
        LambdaMARTParams same;  // the listwise objective's refusals, in LambdaMART's words
        same.objective = p.objective, same.truncation_level = p.truncation_level, same.lambda_norm = p.lambda_norm;
        same.check_objective_options();
        return p;
    }
    Value to_json() const {
        Value o = Value::object();
        o.set("hidden", Value::uint(hidden));
        o.set("num_iterations", Value::uint(num_iterations));
        o.set("learning_rate", Value::number(learning_rate));
        o.set("lambda_l2", Value::number(lambda_l2));
        o.set("sigma", Value::number(sigma));
        o.set("seed", Value::uint(seed));
        o.set("quiet", Value::boolean(quiet));
        if (objective != frdev::M_NDCG) o.set("objective", Value::string(LambdaMARTParams::objective_name(objective)));
        if (truncation_level != 0) o.set("truncation_level", Value::uint(truncation_level));
        if (lambda_norm) o.set("lambda_norm", Value::boolean(true));
        if (trace) o.set("trace", Value::boolean(true));
        if (hidden2 != 0) o.set("hidden2", Value::uint(hidden2));
        return o;
    }
};

constexpr unsigned char ADAM_UPDATED = 1, ADAM_DECAYS = 2;  // a parameter's flags

inline uint64_t neural_init_key(uint64_t seed) { return frresample::mix(seed + 4ull * frresample::GOLDEN); }
inline double neural_init_uniform(uint64_t key, uint64_t c) { return (double)(frresample::mix(key + c) >> 11) * 0x1p-53; }

// The initial net over d columns of which the view holds `feats`, and every parameter's flags in wire order; h2 != 0: with a
// second hidden layer of h2 units.
inline Model neural_init(uint64_t seed, size_t h, size_t d, const std::vector<uint32_t>& feats, std::vector<unsigned char>* flags, size_t h2 = 0) {
    Model m;
    m.kind = Model::NeuralNet;
    m.nn_cols = d;
    const size_t nout = h2 ? h2 : h;  // the output layer's inputs
    m.nn_w1.assign(h * d, 0.0), m.nn_b1.assign(h, 0.0), m.nn_w2.assign(nout, 0.0), m.nn_b2 = 0.0;
    m.nn_hw2.assign(h2 * h, 0.0), m.nn_hb2.assign(h2, 0.0);
    if (flags) flags->assign(h * d + h + h2 * h + h2 + nout + 1, 0);
    const uint64_t key = neural_init_key(seed);
    const double r1 = 6.0 / (double)(feats.size() + h), r2 = 6.0 / (double)(nout + 1);
    const double s1 = std::sqrt(r1), s2 = std::sqrt(r2);
    auto draw = [&](uint64_t c, double scale) {
        const double twice = 2.0 * neural_init_uniform(key, c);
        const double centred = twice - 1.0;
        return centred * scale;
    };
    for (size_t j = 0; j < h; j++) {
        for (uint32_t f : feats) {
            if (f >= d) continue;
            m.nn_w1[j * d + f] = draw(j * d + f, s1);
            if (flags) (*flags)[j * d + f] = ADAM_UPDATED | ADAM_DECAYS;
        }
        if (flags) (*flags)[h * d + j] = ADAM_UPDATED;
    }
    const size_t cw2 = h * d + h, cc = cw2 + h2 * h, cw3 = cc + h2;  // where W2, c and the output weights start
    if (h2 != 0) {
        const double r12 = 6.0 / (double)(h + h2);
        const double s12 = std::sqrt(r12);
        for (size_t c = 0; c < h2 * h; c++) {
            m.nn_hw2[c] = draw(cw2 + c, s12);
            if (flags) (*flags)[cw2 + c] = ADAM_UPDATED | ADAM_DECAYS;
        }
        for (size_t k = 0; flags && k < h2; k++) (*flags)[cc + k] = ADAM_UPDATED;
    }
    for (size_t k = 0; k < nout; k++) {
        m.nn_w2[k] = draw(cw3 + k, s2);
        if (flags) (*flags)[cw3 + k] = ADAM_UPDATED | ADAM_DECAYS;
    }
    if (flags) (*flags)[cw3 + nout] = ADAM_UPDATED;
    return m;
}

// One Adam ascent step (the header comment) over n parameters; flags == nullptr: every parameter is updated and decays.
inline void adam_step(double* theta, const double* grad, double* m, double* v, size_t n, const unsigned char* flags, uint32_t t, double learning_rate,
                      double lambda_l2) {
    const double b1 = 0.9, b2 = 0.999, eps = 1e-8, c1 = 1.0 - b1, c2 = 1.0 - b2;
    double p1 = b1, p2 = b2;
    for (uint32_t k = 1; k < t; k++) p1 = p1 * b1, p2 = p2 * b2;
    const double d1 = 1.0 - p1, d2 = 1.0 - p2;
    for (size_t c = 0; c < n; c++) {
        const unsigned char fl = flags ? flags[c] : (unsigned char)(ADAM_UPDATED | ADAM_DECAYS);
        if (!(fl & ADAM_UPDATED)) continue;
        double g = grad[c];
        if (fl & ADAM_DECAYS) {
            const double reg = lambda_l2 * theta[c];
            g = g - reg;
        }
        const double ma = b1 * m[c], mb = c1 * g;
        m[c] = ma + mb;
        const double gg = g * g;
        const double va = b2 * v[c], vb = c2 * gg;
        v[c] = va + vb;
        const double mh = m[c] / d1, vh = v[c] / d2;
        const double num = learning_rate * mh;
        const double den = std::sqrt(vh) + eps;
        const double step = num / den;
        theta[c] = theta[c] + step;
    }
}

// b: the first iterate (1-based) with the largest measure; 1 when none beats the initial net's (as linear_lambda_best)
inline uint32_t neural_lambda_best(double initial_measure, const std::vector<double>& train_measure) {
    uint32_t best = 0;
    double best_v = initial_measure;
    for (size_t t = 0; t < train_measure.size(); t++)
        if (train_measure[t] > best_v) best = (uint32_t)t + 1, best_v = train_measure[t];
    return best == 0 ? 1u : best;
}

// a net's parameters in wire order, and back
inline std::vector<double> neural_flatten(const Model& m) {
    std::vector<double> th(m.nn_w1);
    th.insert(th.end(), m.nn_b1.begin(), m.nn_b1.end());
    th.insert(th.end(), m.nn_hw2.begin(), m.nn_hw2.end());
    th.insert(th.end(), m.nn_hb2.begin(), m.nn_hb2.end());
    th.insert(th.end(), m.nn_w2.begin(), m.nn_w2.end());
    th.push_back(m.nn_b2);
    return th;
}
inline void neural_unflatten(const std::vector<double>& th, Model* m) {
    const size_t h = m->nn_b1.size(), nw = h * m->nn_cols;
    std::copy(th.begin(), th.begin() + nw, m->nn_w1.begin());
    std::copy(th.begin() + nw, th.begin() + nw + h, m->nn_b1.begin());
    auto at = th.begin() + nw + h;
    for (std::vector<double>* part : {&m->nn_hw2, &m->nn_hb2, &m->nn_w2}) {
        std::copy(at, at + part->size(), part->begin());
        at += part->size();
    }
    m->nn_b2 = *at;
}

inline Value mlp_plan_json(const frdev::DeviceDataset::MlpPlan& plan) {
    Value g = Value::object();
    g.set("feature_panels", Value::uint(plan.feature_panels));
    g.set("hidden_panels", Value::uint(plan.hidden_panels));
    if (plan.hidden2 != 0) g.set("hidden2", Value::uint(plan.hidden2));
    g.set("workgroups", Value::uint(plan.workgroups));
    g.set("stretch_tiles", Value::uint(plan.stretch));
    g.set("tiles", Value::uint(plan.tiles));
    g.set("resident", Value::boolean(plan.resident));
    g.set("slab_bytes", Value::uint(plan.slab_bytes));
    g.set("tile_bytes", Value::uint(plan.tile_bytes));
    return g;
}

struct NeuralLambdaRankStats {
    NeuralLambdaRankParams request;
    uint32_t iterations = 0, best_iteration = 0, features = 0;
    double seconds = 0.0, initial_measure = 0.0;
    double t_score = 0.0, t_gradient = 0.0, t_backprop = 0.0, t_adam = 0.0, t_measure = 0.0;  // wall seconds per stage (device work waited for)
    std::vector<double> train_measure;
    Value initial, iterates = Value::array();  // trace: the initial net and every iterate, as models
    frdev::DeviceDataset::MlpPlan score_plan, backprop_plan;

    Value to_json() const {
        Value o = Value::object();
        o.set("iterations", Value::uint(iterations));
        o.set("best_iteration", Value::uint(best_iteration));
        o.set("features", Value::uint(features));
        o.set("seconds", Value::number(seconds));
        o.set("score_ms", Value::number(t_score * 1e3));
        o.set("gradient_ms", Value::number(t_gradient * 1e3));
        o.set("backprop_ms", Value::number(t_backprop * 1e3));
        o.set("adam_ms", Value::number(t_adam * 1e3));
        o.set("measure_ms", Value::number(t_measure * 1e3));
        o.set("initial_measure", Value::number(initial_measure));
        Value a = Value::array();
        for (double x : train_measure) a.push(Value::number(x));
        o.set("train_measure", std::move(a));
        o.set("request", request.to_json());
        o.set("score_plan", mlp_plan_json(score_plan));
        o.set("backprop_plan", mlp_plan_json(backprop_plan));
        if (request.trace) {
            o.set("initial", initial);
            o.set("iterates", iterates);
        }
        return o;
    }
};

}  // namespace fr
