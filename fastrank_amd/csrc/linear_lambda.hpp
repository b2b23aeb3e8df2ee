// The linear LambdaRank trainer's host side (host only, no HIP): the request's parameters and their wire
// form, the Newton step's solver, the choice of the returned iteration, the statistics.  The loop that drives the device is
// train_linear_lambda.inc.
//
// Definition.  w^0 = 0.  For t = 0 .. num_iterations - 1: the scores of Linear(w^t); one LambdaRank gradient pass on them
// (LambdaMART's, with the same objective keys); H = X^T diag(w) X and g = X^T lambda from the Gram kernel; delta solves
// (H + lambda_l2 I) delta = g; w^(t+1) = w^t + learning_rate * delta (product and sum rounded separately); train_measure[t] =
// the measure's mean of the scores of Linear(w^(t+1)).  The model is Linear(w^b), b the first iteration with the largest
// train_measure; when no iteration beats the all-zero model's measure it is w^1.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "lambdamart.hpp"

namespace fr {

struct LinearLambdaRankParams {
    uint32_t num_iterations = 20;
    double learning_rate = 1.0;
    double lambda_l2 = 1.0;  // (chosen among 1e-6, 1e-3 and 1.0 by training NDCG on the bundled example: DESIGN.md section 18)
    double sigma = 1.0;
    bool quiet = false;
    // the gradient pass's keys, LambdaMART's (optional, not written at their defaults)
    int objective = frdev::M_NDCG;
    uint32_t truncation_level = 0;
    bool lambda_norm = false;

    bool xendcg() const { return objective == frdev::LM_OBJECTIVE_XENDCG; }
    int objective_evaluator() const { return xendcg() ? (int)frdev::M_NDCG : objective; }
    const char* objective_measure() const { return objective == frdev::M_AP ? "ap" : objective == frdev::M_RR ? "rr" : nullptr; }
    frdev::DeviceDataset::LambdaPass pass() const { return {nullptr, false, truncation_level, lambda_norm, objective, 0}; }

    static LinearLambdaRankParams from_json(const Value& v) {
        if (!v.is_object()) fail_raw("Error(\"invalid type: expected struct LinearLambdaRankParams\", line: 0, column: 0)");
        // what the trainer does not do, refused by name where a key suggests it
        const std::pair<const char*, const char*> out_of_scope[] = {
            {"validation_queries", "held-out queries are not supported by LinearLambdaRank (hold them out of the dataset with a query sample)"},
            {"early_stopping_rounds", "held-out queries are not supported by LinearLambdaRank (the best training iteration is returned)"},
            {"init_model", "init_model is not supported by LinearLambdaRank (training starts from all-zero weights)"},
            {"valid", "a validation dataset is not supported by LinearLambdaRank"},
            {"validation_dataset", "a validation dataset is not supported by LinearLambdaRank"}};
        for (const auto& kv : out_of_scope)
            if (v.find(kv.first)) LambdaMARTParams::invalid(kv.second);
        LinearLambdaRankParams p;
        p.num_iterations = json_u32(json_field(v, "num_iterations"), "num_iterations");
        p.learning_rate = json_f64(json_field(v, "learning_rate"), "learning_rate");
        p.lambda_l2 = json_f64(json_field(v, "lambda_l2"), "lambda_l2");
        p.sigma = json_f64(json_field(v, "sigma"), "sigma");
        p.quiet = json_bool(json_field(v, "quiet"), "quiet");
        if (const Value* g = v.find("objective")) p.objective = LambdaMARTParams::objective_from_json(*g);
        if (p.objective == frdev::LM_OBJECTIVE_APPROXNDCG)
            LambdaMARTParams::invalid("objective `approxndcg` is not supported by LinearLambdaRank (its Gram matrix needs the hessian weight w, and the objective's second derivative is not sign-definite; NeuralLambdaRank takes it)");
        if (const Value* r = v.find("truncation_level")) p.truncation_level = json_u32(*r, "truncation_level");
        if (const Value* r = v.find("lambda_norm")) p.lambda_norm = json_bool(*r, "lambda_norm");
        for (const auto& kv : v.obj) {
            static const char* known[] = {"num_iterations", "learning_rate", "lambda_l2", "sigma", "quiet", "objective", "truncation_level", "lambda_norm"};
            bool ok = false;
            for (const char* k : known) ok = ok || kv.first == k;
            if (!ok) fail_raw("Error(\"unknown field `" + kv.first + "` of LinearLambdaRankParams\", line: 0, column: 0)");
        }
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
        o.set("num_iterations", Value::uint(num_iterations));
        o.set("learning_rate", Value::number(learning_rate));
        o.set("lambda_l2", Value::number(lambda_l2));
        o.set("sigma", Value::number(sigma));
        o.set("quiet", Value::boolean(quiet));
        if (objective != frdev::M_NDCG) o.set("objective", Value::string(LambdaMARTParams::objective_name(objective)));
        if (truncation_level != 0) o.set("truncation_level", Value::uint(truncation_level));
        if (lambda_norm) o.set("lambda_norm", Value::boolean(true));
        return o;
    }
};

// delta of (H + lambda_l2 I) delta = g by Cholesky, H row-major n x n (its lower triangle is read).  Fixed order: column by
// column, every inner product summed with k ascending, products and sums rounded separately; then the forward and the backward
// substitution in the same manner.  Returns -1, or the index of the first pivot that is not positive (a NaN one included), in
// which case *pivot holds it and delta is not written.
inline int newton_step(const double* H, const double* g, size_t n, double lambda_l2, double* delta, double* pivot) {
    std::vector<double> L(n * n, 0.0), y(n, 0.0);
    for (size_t j = 0; j < n; j++) {
        double s = H[j * n + j] + lambda_l2;
        for (size_t k = 0; k < j; k++) {
            const double sq = L[j * n + k] * L[j * n + k];
            s = s - sq;
        }
        if (!(s > 0.0) || !std::isfinite(s)) {
            if (pivot) *pivot = s;
            return (int)j;
        }
        const double ljj = std::sqrt(s);
        L[j * n + j] = ljj;
        for (size_t i = j + 1; i < n; i++) {
            double t = H[i * n + j];
            for (size_t k = 0; k < j; k++) {
                const double pr = L[i * n + k] * L[j * n + k];
                t = t - pr;
            }
            L[i * n + j] = t / ljj;
        }
    }
    for (size_t i = 0; i < n; i++) {  // L y = g
        double t = g[i];
        for (size_t k = 0; k < i; k++) {
            const double pr = L[i * n + k] * y[k];
            t = t - pr;
        }
        y[i] = t / L[i * n + i];
    }
    for (size_t ii = n; ii-- > 0;) {  // L^T delta = y
        double t = y[ii];
        for (size_t k = ii + 1; k < n; k++) {
            const double pr = L[k * n + ii] * delta[k];
            t = t - pr;
        }
        delta[ii] = t / L[ii * n + ii];
    }
    return -1;
}

// the plain error of a pivot that is not positive; `feature`: how the caller names column `index`
inline std::string newton_pivot_message(const std::string& feature, double pivot, double lambda_l2) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.17g", pivot);
    char l2[64];
    std::snprintf(l2, sizeof l2, "%.17g", lambda_l2);
    return "LinearLambdaRank: the Newton matrix H + lambda_l2 I is not positive definite at feature " + feature + " (pivot " + buf +
           " under lambda_l2 = " + l2 + "); try a larger lambda_l2";
}

// b: the first iteration (1-based: w^b) with the largest measure; 1 when none beats the all-zero model's
inline uint32_t linear_lambda_best(double zero_measure, const std::vector<double>& train_measure) {
    uint32_t best = 0;
    double best_v = zero_measure;
    for (size_t t = 0; t < train_measure.size(); t++)
        if (train_measure[t] > best_v) best = (uint32_t)t + 1, best_v = train_measure[t];
    return best == 0 ? 1u : best;
}

struct LinearLambdaRankStats {
    LinearLambdaRankParams request;
    uint32_t iterations = 0, best_iteration = 0, features = 0;
    double seconds = 0.0, zero_measure = 0.0;
    double t_score = 0.0, t_gradient = 0.0, t_gram = 0.0, t_solve = 0.0, t_measure = 0.0;  // wall seconds per stage (device work waited for)
    std::vector<double> train_measure;
    std::vector<std::vector<double>> weights;  // w^1 .. w^T, each over the dataset's d columns
    frdev::DeviceDataset::GramPlan plan;

    Value to_json() const {
        Value o = Value::object();
        o.set("iterations", Value::uint(iterations));
        o.set("best_iteration", Value::uint(best_iteration));
        o.set("features", Value::uint(features));
        o.set("seconds", Value::number(seconds));
        o.set("score_ms", Value::number(t_score * 1e3));
        o.set("gradient_ms", Value::number(t_gradient * 1e3));
        o.set("gram_ms", Value::number(t_gram * 1e3));
        o.set("solve_ms", Value::number(t_solve * 1e3));
        o.set("measure_ms", Value::number(t_measure * 1e3));
        o.set("zero_measure", Value::number(zero_measure));
        Value a = Value::array();
        for (double x : train_measure) a.push(Value::number(x));
        o.set("train_measure", std::move(a));
        Value ws = Value::array();
        for (const auto& w : weights) {
            Value r = Value::array();
            for (double x : w) r.push(Value::number(x));
            ws.push(std::move(r));
        }
        o.set("weights", std::move(ws));
        o.set("lambda_l2", Value::number(request.lambda_l2));
        o.set("learning_rate", Value::number(request.learning_rate));
        o.set("objective", Value::string(LambdaMARTParams::objective_name(request.objective)));
        if (request.truncation_level != 0) o.set("truncation_level", Value::uint(request.truncation_level));
        if (request.lambda_norm) o.set("lambda_norm", Value::boolean(true));
        Value g = Value::object();
        g.set("passes", Value::uint(plan.passes));
        g.set("workgroups", Value::uint(plan.workgroups));
        g.set("stretch_tiles", Value::uint(plan.stretch));
        g.set("tiles", Value::uint(plan.tiles));
        g.set("slab_bytes", Value::uint(plan.slab_bytes));
        g.set("tile_bytes", Value::uint(plan.tile_bytes));
        o.set("gram", std::move(g));
        return o;
    }
};

}  // namespace fr
