// Coordinate ascent as the reference runs it (src/coordinate_ascent.rs:11-254): the parameters, one restart's search
// (optimize_inner, :87-195) as a state machine over scores someone else computes, and the selection over the restarts'
// results.  Plain C++ -- no HIP, no device dataset, no environment, no printing: CATrainer (host.hpp) stages a line search,
// has the device score its candidates, hands the scores back to replay() and prints what the two return.
// tests/ca_restart_sanitize.cpp drives it without a device against tests/ca_restart_model.py.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "model.hpp"
#include "rand64.hpp"

namespace fr {

struct CAParams {
    uint32_t num_restarts = 5;
    uint32_t num_max_iterations = 25;
    double step_base = 0.05;
    double step_scale = 2.0;
    double tolerance = 0.001;
    uint64_t seed = 0;
    bool normalize = true;
    bool quiet = false;
    bool init_random = true;
    bool output_ensemble = false;

    static CAParams defaults() {
        CAParams p;
        Rand64 rand(0xdeadbeefULL);
        p.seed = rand.rand_u64();  // coordinate_ascent.rs:27,34
        return p;
    }
    static CAParams from_json(const Value& v) {
        CAParams p;
        p.num_restarts = json_u32(json_field(v, "num_restarts"), "num_restarts");
        p.num_max_iterations = json_u32(json_field(v, "num_max_iterations"), "num_max_iterations");
        p.step_base = json_f64(json_field(v, "step_base"), "step_base");
        p.step_scale = json_f64(json_field(v, "step_scale"), "step_scale");
        p.tolerance = json_f64(json_field(v, "tolerance"), "tolerance");
        p.seed = json_u64(json_field(v, "seed"), "seed");
        p.normalize = json_bool(json_field(v, "normalize"), "normalize");
        p.quiet = json_bool(json_field(v, "quiet"), "quiet");
        p.init_random = json_bool(json_field(v, "init_random"), "init_random");
        p.output_ensemble = json_bool(json_field(v, "output_ensemble"), "output_ensemble");
        return p;
    }
    Value to_json() const {
        Value o = Value::object();
        o.set("num_restarts", Value::uint(num_restarts));
        o.set("num_max_iterations", Value::uint(num_max_iterations));
        o.set("step_base", Value::number(step_base));
        o.set("step_scale", Value::number(step_scale));
        o.set("tolerance", Value::number(tolerance));
        o.set("seed", Value::uint(seed));
        o.set("normalize", Value::boolean(normalize));
        o.set("quiet", Value::boolean(quiet));
        o.set("init_random", Value::boolean(init_random));
        o.set("output_ensemble", Value::boolean(output_ensemble));
        return o;
    }
};

struct RestartResult {
    uint32_t restart_id = 0;
    double score = 0.0;
    std::vector<double> weights;
};

// coordinate_ascent.rs:72-82.  Returns the divisor used: the L1 norm, or 1.0 when that is 0 (w is then left as it is).
inline double l1_normalize(std::vector<double>& w) {
    double sum = 0.0;
    for (double x : w) sum += std::fabs(x);
    if (sum > 0.0) {
        for (double& x : w) x /= sum;
        return sum;
    }
    return 1.0;
}

// Candidate weights of one line search in evaluation order (coordinate_ascent.rs:145-171):
// block 0 = dir 0 (1 candidate), block 1 = dir -1, block 2 = dir +1.
inline void line_candidates(double orig, const CAParams& p, std::vector<double>& out, uint32_t block_len[3]) {
    static const int SIGN[3] = {0, -1, 1};
    out.clear();
    for (int s = 0; s < 3; s++) {
        double dir = (double)SIGN[s];
        double step = p.step_base * dir;
        if (orig != 0.0 && std::fabs(step) > 0.5 * std::fabs(orig)) step = p.step_base * std::fabs(orig) * dir;
        double total = step;
        uint32_t iters = p.num_max_iterations;
        if (SIGN[s] == 0) {
            iters = 1;
            total = -orig;
        }
        block_len[s] = iters;
        for (uint32_t it = 0; it < iters; it++) {
            out.push_back(orig + total);
            step *= p.step_scale;
            total += step;
        }
    }
}

// One restart (optimize_inner).  The caller scores the initial weights into best_score (:110-111), then alternates
// stage() and replay() until `done`.
struct CARestart {
    uint32_t id;
    Rand64 rand;
    std::vector<double> best_w;  // length d (entries the features do not name stay 0)
    double best_score = 0.0;
    std::vector<uint32_t> order;  // this pass's feature order; empty: the next stage() starts a pass
    size_t pos = 0;               // line searches of this pass already replayed
    size_t successes = 0;
    bool done = false;
    // the staged line search
    std::vector<double> base;   // best_w when it was staged, normalised if asked
    std::vector<double> cands;  // values of base[feature] in evaluation order, block_len[s] of them per direction
    uint32_t block_len[3] = {0, 0, 0};
    double start_score = 0.0;
    double norm = 1.0;  // what base was divided by
    struct Accepted {
        size_t cand;  // index into cands
        double score;
    };
    std::vector<Accepted> accepted;  // by the last replay(), in order

    CARestart(uint32_t i, uint64_t seed) : id(i), rand(seed) {}

    // :50-70
    void init_weights(const std::vector<uint32_t>& fids, size_t d, bool init_random) {
        best_w.assign(d, 0.0);
        if (init_random) {
            for (uint32_t f : fids) best_w[f] = rand.rand_float() * 2.0 - 1.0;
        } else {
            for (uint32_t f : fids) best_w[f] = 1.0 / (double)fids.size();
        }
    }

    uint32_t feature() const { return order[pos]; }  // of the staged line search

    // The next line search: a new order at the start of a pass (:113-116), base = best_w, normalised if asked
    // (:134-138), the candidates (:142-171).
    struct Staged {
        uint32_t feature;
        bool new_pass;  // a pass began: best_score is its starting score
    };
    Staged stage(const std::vector<uint32_t>& fids, const CAParams& p) {
        const bool new_pass = pos == 0 && order.empty();
        if (new_pass) {
            order = fids;
            shuffle(order, rand);
            successes = 0;
        }
        start_score = best_score;
        base = best_w;
        norm = p.normalize ? l1_normalize(base) : 1.0;
        line_candidates(base[feature()], p, cands, block_len);
        return {feature(), new_pass};
    }

    struct Replayed {
        size_t evaluated;  // candidates the reference would have scored
        bool finished;     // this line search ended the restart
    };
    // The staged line search over its scores, score_of(c) for candidate c: a candidate replaces the best when its score
    // is not NaN and strictly greater (core.rs:57-66), the directions after one that gained more than the tolerance are
    // skipped (:174), and a pass without such a line search is the last (:179-186).
    template <typename ScoreOf>
    Replayed replay(const CAParams& p, ScoreOf&& score_of) {
        const uint32_t f = feature();
        accepted.clear();
        size_t c = 0;
        for (int s = 0; s < 3; s++) {
            for (uint32_t it = 0; it < block_len[s]; it++, c++) {
                const double sc = score_of(c);
                if (sc == sc && sc > best_score) {
                    best_score = sc;
                    accepted.push_back({c, sc});
                }
            }
            if (best_score - start_score > p.tolerance) break;
        }
        if (!accepted.empty()) {
            best_w = base;
            best_w[f] = cands[accepted.back().cand];
        }
        if (best_score - start_score > p.tolerance) successes++;
        pos++;
        if (pos == order.size()) {
            if (successes == 0) {
                done = true;
            } else {
                pos = 0;
                order.clear();
            }
        }
        return {c, done};
    }
};

// coordinate_ascent.rs:232-252 selection over a restart-ordered history
inline Model ca_select(const std::vector<RestartResult>& hist, bool output_ensemble) {
    if (hist.empty()) fail_str("Should be at least 1 restart!");
    if (output_ensemble && hist.size() > 1) {
        Model ens;
        ens.kind = Model::Ensemble;
        for (const auto& h : hist) {
            Model lin;
            lin.kind = Model::Linear;
            lin.weights = h.weights;
            l1_normalize(lin.weights);
            ens.ens_weights.push_back(h.score);
            ens.members.push_back(std::move(lin));
        }
        return ens;
    }
    size_t best = 0;
    for (size_t k = 0; k < hist.size(); k++)
        if (hist[k].score >= hist[best].score) best = k;  // Iterator::max = last maximum
    Model lin;
    lin.kind = Model::Linear;
    lin.weights = hist[best].weights;
    return lin;
}

}  // namespace fr
