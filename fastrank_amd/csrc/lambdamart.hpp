// LambdaMART on the MI355X path: gradient-boosted regression trees fitted to LambdaRank gradients.
//
// Scores start at 0.0.  Per tree:
//   gradient  lambda_grad_kernel (kernels_lambda.inc) on the running scores in device score slot 0: lambda_p, w_p (f64)
//   grow      the random-forest grower (rf_train.hpp, kernels_rf.inc), SquaredError over ALL of the view's instances and
//             features, fitted to float(lambda_p)
//   leaves    Newton step sum_L lambda / sum_L w over the instances the tree's SCORING rule (x <= split -> lhs) sends to
//             the leaf, both sums sequential f64 in the instance list's order; 0.0 for an empty leaf or sum_L w == 0.
//             The routing is the tree-scoring kernel run on a copy of the tree whose leaves hold their own index.
// grower = "histogram" (lambdamart_hist.hpp, kernels_hist.inc) replaces grow and leaves: features binned once into one byte,
// gradients as int64 fixed point, per-node histograms; leaf values from the leaves' own integer sums.
//   update    s_p = s_p + learning_rate * tree(x_p) (unfused: ensemble_accumulate), the WeightedEnsemble recurrence, so
//             the running scores are what predicting with the model so far gives, bit for bit.
// The instance list is the RF trainer's: queries in the view's order, instance ids ascending inside a query.
// query_sampling_rate / feature_sampling_rate < 1 ("Sampling"): gradient, grow and leaves of a tree
// cover a fresh sample of the queries (a subsequence of the instance list) and of the features, drawn from `seed`; update
// and training measure still cover every document.
// validation_queries ("Validation and early stopping"): the named queries are held out of gradient,
// grow and leaves of every tree (the samples are then drawn from the others); update covers them as well, and the measure
// is reported over the training and the held-out queries separately.  early_stopping_rounds = r > 0 ends training r trees
// after the held-out measure's first maximum and returns the trees up to it.
// split_gain = "newton" (histogram grower only; DESIGN.md section 11, "Newton split gain"): splits are placed by the
// second-order gain G^2 / (H + lambda_l2) with the floors min_sum_hessian and min_split_gain, leaves are G / (H + lambda_l2).
// max_leaves >= 2 (histogram grower only; DESIGN.md section 11, "Leaf-wise growth"): a tree is grown leaf by leaf, the open
// leaf with the largest gain first, until it has max_leaves leaves; 0 (the default) is level-wise growth.
// truncation_level = T >= 1 / lambda_norm (both growers; DESIGN.md section 11, "Truncation and normalisation"): a pair
// contributes to the gradients only when the better ranked of its documents is in the top T, and every query's lambda and
// w are scaled by log2(1 + S_q) / S_q; with either set the gradient stage is lambda_grad_trunc_kernel.
// objective = "map" / "mrr" (both growers; DESIGN.md section 11, "Objectives"): the pair weight is |delta AP| / |delta RR| of
// swapping a relevant and a non-relevant document, and the trainer's evaluator is the AP / RR one: gradient norms, the
// reported measures, the best iteration and early stopping all follow it.  The request's `measure` must still name NDCG.
// drop_rate > 0 (both growers; DESIGN.md section 11, "DART"; lambdamart_dart.hpp): a tree is fitted to the ensemble without a
// random subset of its trees, then it and the dropped trees are re-weighted.  The scores are re-formed from tree 0 by
// dart_rescore_kernel (kernels_dart.inc) from a cache of every (tree, document)'s leaf: after every tree, and once more before
// a tree that drops.
// objective = "xendcg" (both growers; DESIGN.md section 11, "Listwise objective"): the gradients are the listwise cross-entropy
// surrogate's, O(n) per query (lambda_grad_xe_kernel, kernels_xendcg.inc), under a per-tree key k_t of a generator of its own;
// the request's NDCG evaluator keeps every role of the training measure.  truncation_level / lambda_norm are refused.
// monotone_constraints (histogram grower under the Newton gain only; DESIGN.md section 11, "Monotone constraints"): feature
// name -> +1 / -1: with every other feature fixed the model's score never falls / never rises as that feature rises.  Every
// node carries an interval for its output, the scan kernels are the monotone ones, leaves are clamped to their intervals.
// goss_top_rate = a > 0 (histogram grower under the Newton gain only; DESIGN.md section 11, "GOSS"; lambdamart_goss.hpp,
// kernels_goss.inc): a tree is fitted to the a-share of its instance list with the largest |lambda| and to a random
// goss_other_rate-share of the rest, whose lambda and w are multiplied by (1 - a) / b; gradient, update and measure still cover
// every document.  The selection is an on-device radix select under a per-tree key of a generator of its own.
// symmetric_trees (histogram grower, level-wise, no monotone constraints; DESIGN.md section 11, "Symmetric trees"): every node
// of a level splits on the one (feature, threshold) with the largest importance summed over the level's open nodes; a node
// that cannot split under it becomes a leaf.  The trees are ordinary DecisionTrees; everything upstream of the grower composes.
// lambda_l1 / max_delta_step / path_smooth (histogram grower under the Newton gain only; DESIGN.md section 11, "Leaf
// regularisation"; lambdamart_reg.hpp, kernels_histreg.inc): the gradient sum is soft-thresholded before it becomes an output
// or a gain, an output's magnitude is capped, a child's output is pulled toward its parent's; every node carries its output,
// and the scan kernels are the regularised ones.  path_smooth is refused with symmetric_trees.
// grad_quant_bits = b in 2..8 (histogram grower under the Newton gain only; DESIGN.md section 11, "Quantised gradients";
// lambdamart_quant.hpp, kernels_histquant.inc): a tree's fixed-point gradients are rounded stochastically to b bits under a
// per-tree key of a generator of its own, the searches read sums of those small integers (one packed LDS atomic per update in
// the build kernel), and the leaves are renewed from the full-precision sums.  Refused with monotone_constraints, lambda_l1,
// max_delta_step and path_smooth.
// A validation dataset B ("Validation dataset"): a second view, scored tree by tree on its own device form
// (score slot, accumulator, metric pass, mean; under DART a leaf cache of its own); no tree reads it.  Its plain mean over
// all of its queries is the held-out measure the stopping rule reads.
// An init model ("Continued training"): an Ensemble of T0 DecisionTrees.  The scores start at its forest
// scores, new tree j is tree T0 + j of the result and takes every per-tree stream at that index, num_trees counts new trees.
// A request's keys live in LambdaMARTParams alone: the gradient pass and the histogram grower get their options from it
// (pass(), hist_options()), and the stats keep a copy of it (LambdaMARTStats::request) to report from.
#pragma once
#include <chrono>
#include <cmath>
#include <set>
#include <unordered_map>

#include "host.hpp"
#include "lambdamart_dart.hpp"
#include "lambdamart_hist.hpp"
#include "rf_train.hpp"

namespace fr {

// The listwise objective's key stream ("Listwise objective"): tree t's key k_t is the t-th rand_u64()
// of Rand64(seed ^ XENDCG_STREAM); the per-tree samples (Rand64(seed)) and the DART plan (seed ^ DART_STREAM) do not move.
constexpr uint64_t XENDCG_STREAM = 0x58454E4443475845ull;  // "XENDCGXE"

struct LambdaMARTParams {
    uint32_t num_trees = 100;
    double learning_rate = 0.1;
    uint32_t max_depth = 6;
    uint32_t min_leaf_support = 10;
    uint32_t split_candidates = 64;
    double sigma = 1.0;
    bool quiet = false;
    bool histogram = false;  // wire key "grower": "exact" (the default, not written) or "histogram"
    // per-tree samples (optional keys, not written at their defaults): the share of the view's queries a tree is fitted to,
    // the share of the view's features it may split on, the master seed of the samples
    double query_sampling_rate = 1.0, feature_sampling_rate = 1.0;
    uint64_t seed = 0;
    // held-out queries (ids as the dataset spells them) and the stopping rule (optional keys, not written at their defaults)
    std::vector<std::string> validation_queries;
    uint32_t early_stopping_rounds = 0;
    // the split criterion (optional keys, not written at their defaults): wire key "split_gain": "variance" or "newton";
    // the three numbers are read only under "newton"
    bool newton = false;
    double lambda_l2 = 0.0, min_sum_hessian = 0.0, min_split_gain = 0.0;
    // the leaf budget of leaf-wise growth (optional key, not written at its default): 0 = level-wise growth
    uint32_t max_leaves = 0;
    // the objective's truncation level and per-query normalisation (optional keys, not written at their defaults): 0 = every pair
    uint32_t truncation_level = 0;
    bool lambda_norm = false;
    // what the gradients optimise (optional key, not written at its default): frdev::M_NDCG, M_AP ("map", "ap"), M_RR ("mrr", "rr")
    // or frdev::LM_OBJECTIVE_XENDCG ("xendcg": no measure of its own, the NDCG evaluator stays)
    int objective = frdev::M_NDCG;
    // DART (optional keys, not written at their defaults): the chance of every earlier tree to be dropped (0 = plain boosting),
    // the most trees one step drops (0 = no cap), the chance of a step to drop nothing
    double drop_rate = 0.0;
    uint32_t max_drop = 50;
    double skip_drop = 0.5;
    // monotone constraints (optional key, written only when some entry is not 0): feature name (as the dataset spells it) ->
    // +1 / -1, in the request's order; entries of 0 are dropped when the request is read
    std::vector<std::pair<std::string, int>> monotone_constraints;
    // GOSS (optional keys, not written at their defaults): the share of a tree's instances kept for their |lambda| (0 = off),
    // the share of the tree's instances drawn from the others
    double goss_top_rate = 0.0, goss_other_rate = 0.1;
    // symmetric (oblivious) trees (optional key, written only when set): every node of a level splits on the same candidate
    bool symmetric_trees = false;
    // leaf regularisation (optional keys, not written at their defaults; read only under "newton"): the soft threshold of the
    // gradient sum, the cap of an output's magnitude (0 = none), the pull of a child's output toward its parent's (0 = none)
    double lambda_l1 = 0.0, max_delta_step = 0.0, path_smooth = 0.0;
    // quantised gradients (optional key, not written at its default): bits per quantised gradient, 2..8 (0 = off)
    uint32_t grad_quant_bits = 0;

    bool leaf_reg() const { return lambda_l1 != 0.0 || max_delta_step != 0.0 || path_smooth != 0.0; }
    bool goss() const { return goss_top_rate > 0.0; }
    bool dart() const { return drop_rate > 0.0; }
    bool xendcg() const { return objective == frdev::LM_OBJECTIVE_XENDCG; }
    static const char* objective_name(int objective) {
        return objective == frdev::M_AP ? "map" : objective == frdev::M_RR ? "mrr" : objective == frdev::LM_OBJECTIVE_XENDCG ? "xendcg" : "ndcg";
    }
    // the measure whose evaluator the trainer needs under `objective`
    int objective_evaluator() const { return xendcg() ? (int)frdev::M_NDCG : objective; }
    // the evaluator the trainer gets under `objective` (the request's own measure is then read for nothing else)
    const char* objective_measure() const { return objective == frdev::M_AP ? "ap" : objective == frdev::M_RR ? "rr" : nullptr; }
    bool sampling() const { return query_sampling_rate < 1.0 || feature_sampling_rate < 1.0; }
    // a gradient pass under this request: over the flagged queries (nullptr: all), `unchanged` since the pass before;
    // xe_key: the tree's key under "xendcg" (not read otherwise)
    frdev::DeviceDataset::LambdaPass pass(const unsigned char* flags, bool unchanged, uint64_t xe_key = 0) const {
        return {flags, unchanged, truncation_level, lambda_norm, objective, xe_key};
    }
    // what "xendcg" cannot be combined with (the keys speak of pairs, and there are none)
    void check_objective_options() const {
        if (!xendcg()) return;
        if (truncation_level != 0) invalid("truncation_level cannot be combined with objective `xendcg` (a listwise objective has no pairs to truncate)");
        if (lambda_norm) invalid("lambda_norm cannot be combined with objective `xendcg` (a listwise objective has no pair terms to normalise by)");
    }
    // (monotone: the signs resolved against the ascending feature list, lambdamart_monotone_signs; empty without the key)
    HistGrowOptions hist_options(std::vector<int> monotone = {}) const {
        return {split_candidates, max_depth, min_leaf_support, HistNewton{newton, lambda_l2, min_sum_hessian, min_split_gain}, max_leaves,
                std::move(monotone), symmetric_trees, HistReg{lambda_l1, max_delta_step, path_smooth}, grad_quant_bits};
    }
    [[noreturn]] static void invalid(const std::string& what) {
        fail_raw("Error(\"invalid value: " + what + "\", line: 0, column: 0)");
    }
    static int objective_from_json(const Value& g) {
        if (!g.is_string()) fail_raw("Error(\"invalid type: expected a string for objective\", line: 0, column: 0)");
        if (g.s == "ndcg") return frdev::M_NDCG;
        if (g.s == "map" || g.s == "ap") return frdev::M_AP;
        if (g.s == "mrr" || g.s == "rr") return frdev::M_RR;
        if (g.s == "xendcg") return frdev::LM_OBJECTIVE_XENDCG;
        // (the text predates the fourth value and is kept byte for byte: DESIGN.md section 11, "Listwise objective")
        invalid("objective must be `ndcg`, `map` or `mrr`, not `" + g.s + "`");
    }
    // has_valid: the call brings a validation dataset, which is a source of the held-out measure like validation_queries
    static LambdaMARTParams from_json(const Value& v, bool has_valid = false) {
        if (!v.is_object()) fail_raw("Error(\"invalid type: expected struct LambdaMARTParams\", line: 0, column: 0)");
        LambdaMARTParams p;
        p.num_trees = json_u32(json_field(v, "num_trees"), "num_trees");
        p.learning_rate = json_f64(json_field(v, "learning_rate"), "learning_rate");
        p.max_depth = json_u32(json_field(v, "max_depth"), "max_depth");
        p.min_leaf_support = json_u32(json_field(v, "min_leaf_support"), "min_leaf_support");
        p.split_candidates = json_u32(json_field(v, "split_candidates"), "split_candidates");
        p.sigma = json_f64(json_field(v, "sigma"), "sigma");
        p.quiet = json_bool(json_field(v, "quiet"), "quiet");
        if (const Value* g = v.find("grower")) {  // optional (serde: default + skip_serializing_if)
            if (!g->is_string()) fail_raw("Error(\"invalid type: expected a string for grower\", line: 0, column: 0)");
            if (g->s != "exact" && g->s != "histogram") invalid("grower must be `exact` or `histogram`, not `" + g->s + "`");
            p.histogram = g->s == "histogram";
        }
        if (const Value* r = v.find("query_sampling_rate")) p.query_sampling_rate = json_f64(*r, "query_sampling_rate");
        if (const Value* r = v.find("feature_sampling_rate")) p.feature_sampling_rate = json_f64(*r, "feature_sampling_rate");
        if (const Value* r = v.find("seed")) p.seed = json_u64(*r, "seed");
        if (const Value* a = v.find("validation_queries")) {
            if (!a->is_array()) fail_raw("Error(\"invalid type: expected an array of strings for validation_queries\", line: 0, column: 0)");
            std::set<std::string> seen;
            for (const Value& e : a->arr) {
                if (!e.is_string()) fail_raw("Error(\"invalid type: expected a string for every entry of validation_queries\", line: 0, column: 0)");
                if (!seen.insert(e.s).second) invalid("validation_queries names query `" + e.s + "` more than once");
                p.validation_queries.push_back(e.s);
            }
        }
        if (const Value* r = v.find("early_stopping_rounds")) p.early_stopping_rounds = json_u32(*r, "early_stopping_rounds");
        if (const Value* g = v.find("split_gain")) {
            if (!g->is_string()) fail_raw("Error(\"invalid type: expected a string for split_gain\", line: 0, column: 0)");
            if (g->s != "variance" && g->s != "newton") invalid("split_gain must be `variance` or `newton`, not `" + g->s + "`");
            p.newton = g->s == "newton";
        }
        if (const Value* r = v.find("lambda_l2")) p.lambda_l2 = json_f64(*r, "lambda_l2");
        if (const Value* r = v.find("min_sum_hessian")) p.min_sum_hessian = json_f64(*r, "min_sum_hessian");
        if (const Value* r = v.find("min_split_gain")) p.min_split_gain = json_f64(*r, "min_split_gain");
        if (const Value* r = v.find("max_leaves")) p.max_leaves = json_u32(*r, "max_leaves");
        if (const Value* r = v.find("truncation_level")) p.truncation_level = json_u32(*r, "truncation_level");
        if (const Value* r = v.find("lambda_norm")) p.lambda_norm = json_bool(*r, "lambda_norm");
        if (const Value* g = v.find("objective")) p.objective = objective_from_json(*g);
        if (const Value* r = v.find("drop_rate")) p.drop_rate = json_f64(*r, "drop_rate");
        if (const Value* r = v.find("max_drop")) p.max_drop = json_u32(*r, "max_drop");
        if (const Value* r = v.find("skip_drop")) p.skip_drop = json_f64(*r, "skip_drop");
        if (const Value* m = v.find("monotone_constraints")) {
            if (!m->is_object()) fail_raw("Error(\"invalid type: expected an object from feature name to -1, 0 or 1 for monotone_constraints\", line: 0, column: 0)");
            for (const auto& kv : m->obj) {
                const Value& e = kv.second;
                if (e.kind != Value::UInt && e.kind != Value::Int)
                    fail_raw("Error(\"invalid type: expected an integer for every entry of monotone_constraints\", line: 0, column: 0)");
                const bool ok = e.kind == Value::UInt ? e.u <= 1 : (e.i >= -1 && e.i <= 1);
                if (!ok) invalid("monotone_constraints must map feature `" + kv.first + "` to -1, 0 or 1");
                const int sign = e.kind == Value::UInt ? (int)e.u : (int)e.i;
                for (const auto& seen : p.monotone_constraints)
                    if (seen.first == kv.first) invalid("monotone_constraints names feature `" + kv.first + "` more than once");
                if (sign != 0) p.monotone_constraints.emplace_back(kv.first, sign);
            }
        }
        if (const Value* r = v.find("goss_top_rate")) p.goss_top_rate = json_f64(*r, "goss_top_rate");
        if (const Value* r = v.find("goss_other_rate")) p.goss_other_rate = json_f64(*r, "goss_other_rate");
        if (const Value* r = v.find("symmetric_trees")) p.symmetric_trees = json_bool(*r, "symmetric_trees");
        if (const Value* r = v.find("lambda_l1")) p.lambda_l1 = json_f64(*r, "lambda_l1");
        if (const Value* r = v.find("max_delta_step")) p.max_delta_step = json_f64(*r, "max_delta_step");
        if (const Value* r = v.find("path_smooth")) p.path_smooth = json_f64(*r, "path_smooth");
        if (const Value* r = v.find("grad_quant_bits")) p.grad_quant_bits = json_u32(*r, "grad_quant_bits");
        if (p.num_trees < 1) invalid("num_trees must be at least 1");
        if (!(std::isfinite(p.learning_rate) && p.learning_rate > 0.0)) invalid("learning_rate must be finite and greater than 0");
        if (p.max_depth < 1) invalid("max_depth must be at least 1");
        if (!(std::isfinite(p.sigma) && p.sigma > 0.0)) invalid("sigma must be finite and greater than 0");
        if (!(p.query_sampling_rate > 0.0 && p.query_sampling_rate <= 1.0))
            invalid("query_sampling_rate must be greater than 0 and at most 1");
        if (!(p.feature_sampling_rate > 0.0 && p.feature_sampling_rate <= 1.0))
            invalid("feature_sampling_rate must be greater than 0 and at most 1");
        if (p.histogram && (p.split_candidates < 2 || p.split_candidates > 256))
            invalid("split_candidates must be between 2 and 256 for the histogram grower (bins are one byte)");
        if (p.early_stopping_rounds > 0 && p.validation_queries.empty() && !has_valid)
            invalid("early_stopping_rounds needs at least one validation query (validation_queries is empty)");
        if (p.newton && !p.histogram) invalid("split_gain `newton` needs grower: \"histogram\" (the exact grower keeps the random-forest criterion)");
        const std::pair<const char*, double> numbers[] = {{"lambda_l2", p.lambda_l2}, {"min_sum_hessian", p.min_sum_hessian}, {"min_split_gain", p.min_split_gain}};
        for (const auto& kv : numbers) {
            if (!(std::isfinite(kv.second) && kv.second >= 0.0)) invalid(std::string(kv.first) + " must be finite and at least 0");
            if (kv.second != 0.0 && !p.newton) invalid(std::string(kv.first) + " needs split_gain: \"newton\"");
        }
        if (p.max_leaves == 1) invalid("max_leaves must be 0 (level-wise) or at least 2");
        if (p.max_leaves >= 2 && !p.histogram) invalid("max_leaves needs grower: \"histogram\" (the exact grower grows level by level)");
        if (!(p.drop_rate >= 0.0 && p.drop_rate <= 1.0)) invalid("drop_rate must be at least 0 and at most 1");
        if (!(p.skip_drop >= 0.0 && p.skip_drop <= 1.0)) invalid("skip_drop must be at least 0 and at most 1");
        if (p.max_drop != 50 && !p.dart()) invalid("max_drop needs drop_rate greater than 0");
        if (p.skip_drop != 0.5 && !p.dart()) invalid("skip_drop needs drop_rate greater than 0");
        if (p.early_stopping_rounds > 0 && p.dart())
            invalid("early_stopping_rounds cannot be combined with drop_rate greater than 0 (earlier trees' weights keep changing: the trees up to the best iteration are not a model the training measured)");
        if (!p.monotone_constraints.empty() && !p.histogram)
            invalid("monotone_constraints needs grower: \"histogram\" (the exact grower has no hessian sums)");
        if (!p.monotone_constraints.empty() && !p.newton)
            invalid("monotone_constraints needs split_gain: \"newton\" (the variance criterion has no hessian sums)");
        if (!(std::isfinite(p.goss_top_rate) && p.goss_top_rate >= 0.0 && p.goss_top_rate < 1.0))
            invalid("goss_top_rate must be finite, at least 0 and less than 1");
        if (!(std::isfinite(p.goss_other_rate) && p.goss_other_rate > 0.0 && p.goss_other_rate <= 1.0))
            invalid("goss_other_rate must be finite, greater than 0 and at most 1");
        if (!(p.goss_top_rate + p.goss_other_rate <= 1.0)) invalid("goss_top_rate + goss_other_rate must be at most 1");
        if (p.goss_other_rate != 0.1 && !p.goss()) invalid("goss_other_rate needs goss_top_rate greater than 0");
        if (p.goss() && !p.histogram) invalid("goss_top_rate needs grower: \"histogram\" (the exact grower has no hessian sums)");
        if (p.goss() && !p.newton)
            invalid("goss_top_rate needs split_gain: \"newton\" (the variance criterion divides by counts, which amplification does not reach)");
        if (p.symmetric_trees && !p.histogram)
            invalid("symmetric_trees needs grower: \"histogram\" (the exact grower searches every node on its own)");
        if (p.symmetric_trees && p.max_leaves != 0)
            invalid("symmetric_trees cannot be combined with max_leaves (a symmetric tree is grown level by level)");
        if (p.symmetric_trees && !p.monotone_constraints.empty())
            invalid("symmetric_trees cannot be combined with monotone_constraints (a level's one split cannot honour every node's interval)");
        const std::pair<const char*, double> leaf_numbers[] = {{"lambda_l1", p.lambda_l1}, {"max_delta_step", p.max_delta_step}, {"path_smooth", p.path_smooth}};
        for (const auto& kv : leaf_numbers) {
            if (!(std::isfinite(kv.second) && kv.second >= 0.0)) invalid(std::string(kv.first) + " must be finite and at least 0");
            if (kv.second != 0.0 && !p.histogram) invalid(std::string(kv.first) + " needs grower: \"histogram\" (the exact grower has no hessian sums)");
            if (kv.second != 0.0 && !p.newton) invalid(std::string(kv.first) + " needs split_gain: \"newton\"");
        }
        if (p.path_smooth != 0.0 && p.symmetric_trees)
            invalid("path_smooth cannot be combined with symmetric_trees (a level's one split is priced over every node, each with a parent of its own)");
        if (!quant_bits_ok(p.grad_quant_bits)) invalid("grad_quant_bits must be 0 (off) or between 2 and 8");
        if (p.grad_quant_bits != 0) {
            if (!p.histogram) invalid("grad_quant_bits needs grower: \"histogram\" (the exact grower builds no histograms)");
            if (!p.newton) invalid("grad_quant_bits needs split_gain: \"newton\" (the variance criterion has no hessian sums to quantise)");
            const char* undecided = " (their nodes carry outputs computed from sums, and it is not decided whether those would read the quantised sums or the full-precision ones)";
            if (!p.monotone_constraints.empty()) invalid(std::string("grad_quant_bits cannot be combined with monotone_constraints") + undecided);
            for (const auto& kv : leaf_numbers)
                if (kv.second != 0.0) invalid(std::string("grad_quant_bits cannot be combined with ") + kv.first + undecided);
        }
        p.check_objective_options();
        return p;
    }
    Value to_json() const {
        Value o = Value::object();
        o.set("num_trees", Value::uint(num_trees));
        o.set("learning_rate", Value::number(learning_rate));
        o.set("max_depth", Value::uint(max_depth));
        o.set("min_leaf_support", Value::uint(min_leaf_support));
        o.set("split_candidates", Value::uint(split_candidates));
        o.set("sigma", Value::number(sigma));
        o.set("quiet", Value::boolean(quiet));
        if (histogram) o.set("grower", Value::string("histogram"));
        if (query_sampling_rate != 1.0) o.set("query_sampling_rate", Value::number(query_sampling_rate));
        if (feature_sampling_rate != 1.0) o.set("feature_sampling_rate", Value::number(feature_sampling_rate));
        if (seed != 0) o.set("seed", Value::uint(seed));
        if (!validation_queries.empty()) {
            Value a = Value::array();
            for (const std::string& q : validation_queries) a.push(Value::string(q));
            o.set("validation_queries", std::move(a));
        }
        if (early_stopping_rounds != 0) o.set("early_stopping_rounds", Value::uint(early_stopping_rounds));
        if (newton) o.set("split_gain", Value::string("newton"));
        if (lambda_l2 != 0.0) o.set("lambda_l2", Value::number(lambda_l2));
        if (min_sum_hessian != 0.0) o.set("min_sum_hessian", Value::number(min_sum_hessian));
        if (min_split_gain != 0.0) o.set("min_split_gain", Value::number(min_split_gain));
        if (max_leaves != 0) o.set("max_leaves", Value::uint(max_leaves));
        if (truncation_level != 0) o.set("truncation_level", Value::uint(truncation_level));
        if (lambda_norm) o.set("lambda_norm", Value::boolean(true));
        if (objective != frdev::M_NDCG) o.set("objective", Value::string(objective_name(objective)));
        if (drop_rate != 0.0) o.set("drop_rate", Value::number(drop_rate));
        if (max_drop != 50) o.set("max_drop", Value::uint(max_drop));
        if (skip_drop != 0.5) o.set("skip_drop", Value::number(skip_drop));
        if (!monotone_constraints.empty()) {
            Value m = Value::object();
            for (const auto& kv : monotone_constraints) m.set(kv.first, Value::sint(kv.second));
            o.set("monotone_constraints", std::move(m));
        }
        if (goss_top_rate != 0.0) o.set("goss_top_rate", Value::number(goss_top_rate));
        if (goss_other_rate != 0.1) o.set("goss_other_rate", Value::number(goss_other_rate));
        if (symmetric_trees) o.set("symmetric_trees", Value::boolean(true));
        if (lambda_l1 != 0.0) o.set("lambda_l1", Value::number(lambda_l1));
        if (max_delta_step != 0.0) o.set("max_delta_step", Value::number(max_delta_step));
        if (path_smooth != 0.0) o.set("path_smooth", Value::number(path_smooth));
        if (grad_quant_bits != 0) o.set("grad_quant_bits", Value::uint(grad_quant_bits));
        return o;
    }
};

// the measures LambdaMART has gradients for: ndcg and ndcg@k (checked before any device work)
inline void lambdamart_check_measure(const std::string& measure) {
    std::string base = measure.substr(0, measure.find('@'));
    for (auto& ch : base) ch = (char)std::tolower((unsigned char)ch);
    if (base != "ndcg")
        fail_str("LambdaMART: unsupported training measure \"" + measure + "\" (supported: ndcg, ndcg@k)");
}

// the instance list: queries in the view's order, ids ascending inside each (RFTrainer's order)
inline std::vector<uint32_t> lambdamart_instance_list(const frdev::HostCSR& csr) {
    std::vector<uint32_t> ids;
    ids.reserve(csr.n);
    for (size_t qi = 0; qi < csr.nq; qi++) {
        const size_t b = ids.size();
        ids.insert(ids.end(), csr.perm.begin() + csr.qoff[qi], csr.perm.begin() + csr.qoff[qi + 1]);
        std::sort(ids.begin() + b, ids.end());
    }
    return ids;
}

// The split of the view's queries Q (its order) into held-out H and training T = Q \ H, both as ascending indices into Q.
// Host only: a request is checked by this before any device work.
struct LambdaSplit {
    std::vector<uint32_t> train, held;
};
inline LambdaSplit lambdamart_split(DatasetView& view, const LambdaMARTParams& p) {
    const size_t nq = view.host_csr().nq;
    LambdaSplit sp;
    std::vector<unsigned char> out(nq, 0);
    if (!p.validation_queries.empty()) {
        std::unordered_map<std::string, uint32_t> index;
        for (size_t q = 0; q < nq; q++) index.emplace(view.core->qnames[view.csr_query[q]], (uint32_t)q);
        for (const std::string& id : p.validation_queries) {
            auto it = index.find(id);
            if (it == index.end()) LambdaMARTParams::invalid("validation_queries names `" + id + "`, which is not a query of the dataset");
            out[it->second] = 1;  // (repeated ids were refused when the request was parsed)
        }
        if (p.validation_queries.size() >= nq) LambdaMARTParams::invalid("validation_queries holds out every query: no training query left");
    }
    for (size_t q = 0; q < nq; q++) (out[q] ? sp.held : sp.train).push_back((uint32_t)q);
    return sp;
}

// The request's monotone constraints against the view: one sign per entry of the view's ascending feature list `feats`
// (empty without the key).  Host only: a name the view does not hold fails before any device work.
inline std::vector<int> lambdamart_monotone_signs(const DatasetView& view, const std::vector<uint32_t>& feats, const LambdaMARTParams& p) {
    if (p.monotone_constraints.empty()) return {};
    std::vector<int> signs(feats.size(), 0);
    for (const auto& kv : p.monotone_constraints) {
        size_t at = feats.size();
        for (size_t i = 0; i < feats.size() && at == feats.size(); i++)
            if (view.core->feature_name(feats[i]) == kv.first) at = i;
        if (at == feats.size()) LambdaMARTParams::invalid("monotone_constraints names `" + kv.first + "`, which is not a feature of the dataset");
        signs[at] = kv.second;
    }
    return signs;
}

// A tree's sample ("Sampling"): indices into the view's ascending feature list and into the view's
// queries, both ascending.  The master generator Rand64(seed) gives every tree two seeds in order, fseed_t then qseed_t;
// a list is shuffle(0..len-1) under its own Rand64, the first sample_count(len, rate) entries, sorted.  A rate of 1.0 skips
// the shuffle (the full list) but not the seed.  With held-out queries the query list is drawn over 0..|T|-1 and mapped
// through T (`train`): the result is still ascending indices of the view's queries.
struct LambdaSample {
    std::vector<uint32_t> features, queries;
};
inline std::vector<uint32_t> lambdamart_sample_list(uint64_t seed, size_t len, double rate) {
    std::vector<uint32_t> v(len);
    for (size_t i = 0; i < len; i++) v[i] = (uint32_t)i;
    if (rate >= 1.0) return v;
    Rand64 local(seed);
    shuffle(v, local);
    v.resize(sample_count(len, rate));
    std::sort(v.begin(), v.end());
    return v;
}
inline LambdaSample lambdamart_next_sample(Rand64& master, size_t n_features, size_t n_queries, const LambdaMARTParams& p,
                                           const std::vector<uint32_t>* train = nullptr) {
    const uint64_t fseed = master.rand_u64(), qseed = master.rand_u64();
    LambdaSample smp{lambdamart_sample_list(fseed, n_features, p.feature_sampling_rate),
                     lambdamart_sample_list(qseed, train ? train->size() : n_queries, p.query_sampling_rate)};
    if (train)
        for (uint32_t& q : smp.queries) q = (*train)[q];
    return smp;
}

// A validation dataset against the training view and the request (host only: refused before any device work).
inline void lambdamart_check_valid(DatasetView& view, DatasetView& valid, const LambdaMARTParams& p) {
    if (!p.validation_queries.empty())
        LambdaMARTParams::invalid("validation_queries cannot be combined with a validation dataset (there is one source of the held-out measure)");
    bool all_a = true, all_b = true;
    DatasetView *own_a = view.matrix_owner(&all_a), *own_b = valid.matrix_owner(&all_b);
    if (&view == &valid || (own_a == own_b && all_a && all_b))
        LambdaMARTParams::invalid("the validation dataset is the dataset being trained on (hold queries of it out with validation_queries)");
    std::set<uint32_t> have(valid.features.begin(), valid.features.end());
    std::vector<uint32_t> feats = view.features;
    std::sort(feats.begin(), feats.end());
    for (uint32_t f : feats)
        if (!have.count(f))
            LambdaMARTParams::invalid("the validation dataset does not hold feature `" + view.core->feature_name(f) + "` of the training dataset");
    if (valid.host_csr().nq == 0) LambdaMARTParams::invalid("the validation dataset holds no query");
    const int da = view.built_on_device(), db = valid.built_on_device();
    if (da >= 0 && db >= 0 && da != db)
        LambdaMARTParams::invalid("the validation dataset lives on device " + std::to_string(db) + ", the training dataset on device " +
                                  std::to_string(da) + " (a validation dataset on another device is not supported)");
}

// An init model against the request (host only): an Ensemble of DecisionTrees with finite numbers, one weight per tree.
inline void lambdamart_check_init(const Model& m, const LambdaMARTParams& p) {
    auto refuse = [](const std::string& what) { fail_str("LambdaMART: init_model must be an Ensemble of DecisionTrees, not " + what); };
    if (m.kind == Model::Linear) refuse("a Linear model");
    if (m.kind == Model::SingleFeature) refuse("a SingleFeature model");
    if (m.kind == Model::DecisionTree) refuse("a bare DecisionTree (wrap it in an Ensemble with a weight)");
    if (m.members.size() != m.ens_weights.size())
        fail_str("LambdaMART: init_model has " + std::to_string(m.ens_weights.size()) + " weights for " + std::to_string(m.members.size()) + " models");
    for (size_t t = 0; t < m.members.size(); t++) {
        const Model& mm = m.members[t];
        if (mm.kind == Model::Ensemble) refuse("an Ensemble with a nested Ensemble (member " + std::to_string(t) + ")");
        if (mm.kind != Model::DecisionTree) refuse(std::string("an Ensemble with a ") + (mm.kind == Model::Linear ? "Linear" : "SingleFeature") + " member (member " + std::to_string(t) + ")");
        if (!std::isfinite(m.ens_weights[t])) fail_str("LambdaMART: init_model has a non-finite weight (tree " + std::to_string(t) + ")");
        std::vector<const TreeNode*> work{mm.tree.get()};
        while (!work.empty()) {
            const TreeNode* n = work.back();
            work.pop_back();
            if (!n) fail_str("LambdaMART: init_model has an empty tree (tree " + std::to_string(t) + ")");
            if (!std::isfinite(n->value))
                fail_str(std::string("LambdaMART: init_model has a non-finite ") + (n->leaf ? "leaf" : "split") + " (tree " + std::to_string(t) + ")");
            if (!n->leaf) work.push_back(n->lhs.get()), work.push_back(n->rhs.get());
        }
    }
    if (p.dart())
        LambdaMARTParams::invalid("init_model cannot be combined with drop_rate greater than 0 (dropping or re-weighting the given trees needs their leaf caches and changes a model the caller owns)");
}

struct LambdaMARTStats {
    LambdaMARTParams request;  // what was asked for: the keys reported below are read from it
    uint32_t trees = 0;
    double seconds = 0.0;
    double t_gradient = 0.0, t_grow = 0.0, t_leaves = 0.0, t_update = 0.0;  // wall seconds per stage (device work waited for)
    std::vector<double> train_measure;                                        // evaluator mean of the running scores after each tree
    double t_bins = 0.0;   // one-off binning (0 when the view's kept bins were reused, and for the exact grower)
    // per-tree samples (reported only when a rate is below 1, with the request's keys): the trees' summed sample sizes
    uint64_t sum_queries = 0, sum_instances = 0, sum_features = 0;
    // held-out queries (reported only when there are any): with them train_measure is the mean over the training queries
    bool stopped_early = false;
    uint32_t validation_queries = 0, training_queries = 0, best_iteration = 0;
    std::vector<double> valid_measure;  // evaluator mean of the running scores over the held-out queries after each tree
    // leaf-wise growth (reported only when max_leaves is set): the trees' summed numbers of leaves, and the histogram pool
    // (slots x the tree's features x bins x 12 or 20 B), the largest over the trees
    uint64_t sum_leaves = 0, pool_bytes = 0;
    // DART (reported only when drop_rate > 0): the trees each tree was fitted without, the wall seconds of the re-formings of
    // the scores and of the leaf cache's fills (kept out of t_update), the cache's bytes
    std::vector<uint32_t> dropped;
    double t_dart = 0.0;
    uint64_t dart_cache_bytes = 0;
    // monotone constraints (reported only when the key is set): feature id -> sign, and per tree the leaves a bound moved
    std::vector<std::pair<uint32_t, int>> monotone;
    std::vector<uint32_t> clamped_leaves;
    // GOSS (reported only when goss_top_rate > 0): the wall seconds of making the trees' lists (a share of t_grow), and per
    // tree the list's length n_g and the top set's size n_top
    double t_goss = 0.0;
    std::vector<uint32_t> goss_instances, goss_top;
    // symmetric trees (reported only when the key is set): per tree the levels that split
    std::vector<uint32_t> levels;
    // quantised gradients (reported only when grad_quant_bits is set): the wall seconds of the quantise launches (a share of t_grow)
    double t_quant = 0.0;
    double best_valid_measure = 0.0;  // the held-out measure at best_iteration
    // a validation dataset (reported only when one is given): its sizes and the wall seconds of its side of every tree
    bool valid_dataset = false;
    uint32_t valid_dataset_queries = 0, valid_dataset_instances = 0;
    double t_valid = 0.0;
    uint64_t valid_dart_cache_bytes = 0;  // under DART: the bytes of the validation dataset's own leaf cache
    // an init model (reported only when one is given): its trees, the measures of its scores, the wall seconds of forming them
    bool init_model = false;
    uint32_t init_trees = 0;
    double init_train_measure = 0.0, init_valid_measure = 0.0, t_init = 0.0;

    Value to_json() const {
        const LambdaMARTParams& r = request;
        Value o = Value::object();
        o.set("trees", Value::uint(trees));
        o.set("seconds", Value::number(seconds));
        o.set("gradient_ms", Value::number(t_gradient * 1e3));
        o.set("grow_ms", Value::number(t_grow * 1e3));
        o.set("leaves_ms", Value::number(t_leaves * 1e3));
        o.set("update_ms", Value::number(t_update * 1e3));
        o.set("grower", Value::string(r.histogram ? "histogram" : "exact"));
        o.set("bins_ms", Value::number(t_bins * 1e3));
        if (r.histogram) o.set("bins", Value::uint(r.split_candidates));
        if (r.sampling()) {
            const double T = trees ? (double)trees : 1.0;
            o.set("query_sampling_rate", Value::number(r.query_sampling_rate));
            o.set("feature_sampling_rate", Value::number(r.feature_sampling_rate));
            o.set("seed", Value::uint(r.seed));
            o.set("sample_queries", Value::number((double)sum_queries / T));
            o.set("sample_instances", Value::number((double)sum_instances / T));
            o.set("sample_features", Value::number((double)sum_features / T));
        }
        Value a = Value::array();
        for (double x : train_measure) a.push(Value::number(x));
        o.set("train_measure", std::move(a));
        if (validation_queries != 0 || valid_dataset) {
            if (valid_dataset) {
                o.set("valid_dataset_queries", Value::uint(valid_dataset_queries));
                o.set("valid_dataset_instances", Value::uint(valid_dataset_instances));
                o.set("valid_ms", Value::number(t_valid * 1e3));
                if (r.dart()) o.set("valid_dart_cache_bytes", Value::uint(valid_dart_cache_bytes));
            } else {
                o.set("validation_queries", Value::uint(validation_queries));
                o.set("training_queries", Value::uint(training_queries));
            }
            Value b = Value::array();
            for (double x : valid_measure) b.push(Value::number(x));
            o.set("valid_measure", std::move(b));
            o.set("best_iteration", Value::uint(best_iteration));
            o.set("best_valid_measure", Value::number(best_valid_measure));
            o.set("stopped_early", Value::boolean(stopped_early));
            o.set("early_stopping_rounds", Value::uint(r.early_stopping_rounds));
        }
        if (init_model) {
            o.set("init_trees", Value::uint(init_trees));
            o.set("init_train_measure", Value::number(init_train_measure));
            if (validation_queries != 0 || valid_dataset) o.set("init_valid_measure", Value::number(init_valid_measure));
            o.set("init_ms", Value::number(t_init * 1e3));
        }
        // (the Newton gain and the leaf budget are the histogram grower's: a request sets them with no other)
        if (r.histogram && r.newton) {
            o.set("split_gain", Value::string("newton"));
            o.set("lambda_l2", Value::number(r.lambda_l2));
            o.set("min_sum_hessian", Value::number(r.min_sum_hessian));
            o.set("min_split_gain", Value::number(r.min_split_gain));
        }
        if (r.histogram && r.max_leaves != 0) {
            o.set("max_leaves", Value::uint(r.max_leaves));
            o.set("mean_leaves", Value::number((double)sum_leaves / (trees ? (double)trees : 1.0)));
            o.set("pool_bytes", Value::uint(pool_bytes));
        }
        if (r.truncation_level != 0) o.set("truncation_level", Value::uint(r.truncation_level));
        if (r.lambda_norm) o.set("lambda_norm", Value::boolean(true));
        if (r.objective != frdev::M_NDCG) o.set("objective", Value::string(LambdaMARTParams::objective_name(r.objective)));
        if (r.dart()) {
            o.set("drop_rate", Value::number(r.drop_rate));
            o.set("max_drop", Value::uint(r.max_drop));
            o.set("skip_drop", Value::number(r.skip_drop));
            Value k = Value::array();
            for (uint32_t x : dropped) k.push(Value::uint(x));
            o.set("dropped", std::move(k));
            o.set("dart_ms", Value::number(t_dart * 1e3));
            o.set("dart_cache_bytes", Value::uint(dart_cache_bytes));
        }
        if (!r.monotone_constraints.empty()) {
            Value m = Value::object();
            for (const auto& kv : monotone) m.set(std::to_string(kv.first), Value::sint(kv.second));
            o.set("monotone_constraints", std::move(m));
            Value k = Value::array();
            for (uint32_t x : clamped_leaves) k.push(Value::uint(x));
            o.set("monotone_clamped_leaves", std::move(k));
        }
        if (r.goss()) {
            o.set("goss_top_rate", Value::number(r.goss_top_rate));
            o.set("goss_other_rate", Value::number(r.goss_other_rate));
            o.set("goss_ms", Value::number(t_goss * 1e3));
            Value a = Value::array(), b = Value::array();
            for (uint32_t x : goss_instances) a.push(Value::uint(x));
            for (uint32_t x : goss_top) b.push(Value::uint(x));
            o.set("goss_instances", std::move(a));
            o.set("goss_top", std::move(b));
        }
        if (r.symmetric_trees) {
            o.set("symmetric_trees", Value::boolean(true));
            Value a = Value::array();
            for (uint32_t x : levels) a.push(Value::uint(x));
            o.set("levels", std::move(a));
        }
        if (r.leaf_reg()) {
            o.set("lambda_l1", Value::number(r.lambda_l1));
            o.set("max_delta_step", Value::number(r.max_delta_step));
            o.set("path_smooth", Value::number(r.path_smooth));
        }
        if (r.grad_quant_bits != 0) {
            o.set("grad_quant_bits", Value::uint(r.grad_quant_bits));
            o.set("quant_ms", Value::number(t_quant * 1e3));
        }
        return o;
    }
};

class LambdaMARTTrainer {
  public:
    LambdaMARTTrainer(std::shared_ptr<DatasetView> view, Evaluator ev, LambdaMARTParams p)
        : view_(std::move(view)), ev_(std::move(ev)), p_(p) {}
    // a validation dataset with its own evaluator (the request's measure and judgments over ITS queries)
    void set_valid(std::shared_ptr<DatasetView> valid, Evaluator ev) { valid_ = std::move(valid), vev_ = std::move(ev); }
    // the model training continues from (checked by lambdamart_check_init; must outlive learn())
    void set_init(const Model* init) { init_ = init; }

    Model learn() {
        auto t0 = std::chrono::steady_clock::now();
        stats_.request = p_;
        auto tnow = [] { return std::chrono::steady_clock::now(); };
        auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
            return std::chrono::duration<double>(b - a).count();
        };
        // gradients exist for NDCG, AP and RR, and the evaluator must be the objective's: the kernels read its norms
        // (the listwise objective keeps the NDCG evaluator)
        if (ev_.measure != p_.objective_evaluator())
            fail_str(std::string("LambdaMART: the evaluator does not belong to the objective `") + LambdaMARTParams::objective_name(p_.objective) + "`");
        const LambdaSplit split = lambdamart_split(*view_, p_);  // (host only: a bad list fails before any device work)
        const bool hold = !split.held.empty();
        const bool vd = (bool)valid_;                      // a validation dataset: `hold` is then false (checked)
        const bool held_measure = hold || vd;              // there is a held-out measure for the stopping rule
        const uint32_t T0 = init_ ? (uint32_t)init_->members.size() : 0u;
        if (vd) lambdamart_check_valid(*view_, *valid_, p_);
        if (init_) lambdamart_check_init(*init_, p_);
        if (vd && vev_.measure != ev_.measure) fail_str("LambdaMART: the validation dataset's evaluator is not the training one's");
        std::vector<uint32_t> feats = view_->features;
        std::sort(feats.begin(), feats.end());
        const std::vector<int> signs = lambdamart_monotone_signs(*view_, feats, p_);  // (host only as well)
        for (size_t i = 0; i < signs.size(); i++)
            if (signs[i] != 0) stats_.monotone.emplace_back(feats[i], signs[i]);
        frdev::DeviceDataset& dev = view_->device();
        const frdev::HostCSR& csr = view_->host_csr();
        const DataCore& core = *view_->core;
        std::string err;
        if (feats.empty()) fail_str("assertion failed: !features.is_empty()");
        if (csr.nq == 0) fail_str("assertion failed: !data.queries().is_empty()");
        // the instance list: queries in the view's order, ids ascending inside each (RFTrainer's order)
        const std::vector<uint32_t> root_ids = lambdamart_instance_list(csr);
        if (!p_.histogram && (uint64_t)root_ids.size() * feats.size() >= (1ull << 31))
            fail_str("LambdaMART: instances x features exceeds the device sort's index range");
        const std::vector<uint32_t> root_off = {0u, (uint32_t)root_ids.size()};
        std::vector<uint32_t> positions(root_ids.size());
        if (!dev.rf_positions(root_ids, positions.data(), &err)) fail_str(err);
        if (!p_.histogram && !dev.rf_set_presence(core.present_bits.empty() ? nullptr : core.present_bits.data(), core.present_words, core.n, &err))
            fail_str(err);
        uint32_t max_id = 0;
        for (uint32_t id : root_ids) max_id = std::max(max_id, id);

        std::unique_ptr<HistGrower> hist;
        if (p_.histogram) {
            hist.reset(new HistGrower(dev, feats, p_.hist_options(signs)));
            auto tb0 = tnow();
            if (hist->prepare(positions)) stats_.t_bins = secs(tb0, tnow());
        }
        // Non-finite feature values are refused, whichever grower: the histogram grower's edges are data values, so -inf can
        // become a split, and the exact grower puts +inf where the reference's position rule does (random_forest.rs:238) --
        // a tree that to_json writes as null, init_model refuses and explain refuses.  (A NaN under the histogram grower has
        // failed above with the binning's own message.)  Read from the device form's per-column max |x|, which a query view
        // inherits from the dataset it was sampled from: a view is refused by its parent's column.
        {
            const std::vector<double>& absmax = dev.column_absmax();
            for (uint32_t f : feats)
                if (f < absmax.size() && !std::isfinite(absmax[f]))
                    fail_str("LambdaMART: feature " + std::to_string(f) + " holds an inf or NaN value (in this dataset, or in the dataset it is a query "
                             "view of); trees are only trained on finite feature values");
        }
        RFParams rp;
        rp.quiet = true;
        rp.num_trees = 1;
        rp.weight_trees = false;
        rp.split_method = 0;
        rp.min_leaf_support = p_.min_leaf_support;
        rp.split_candidates = p_.split_candidates;
        rp.max_depth = p_.max_depth;
        RFTrainer grower(view_, ev_, rp);
        RFStats rst;
        struct EndGuard {
            frdev::DeviceDataset& d;
            ~EndGuard() { d.rf_end(), d.subset_means_end(); }
        } end_guard{dev};
        // the validation dataset's device form, on the training view's device (built there when it does not exist yet)
        frdev::DeviceDataset* vdev = nullptr;
        if (vd) {
            if (!frdev::set_device(dev.device_ordinal(), &err)) fail_str(err);
            vdev = &valid_->device();
            if (vdev == &dev) LambdaMARTParams::invalid("the validation dataset is the dataset being trained on (hold queries of it out with validation_queries)");
            if (vdev->device_ordinal() != dev.device_ordinal())
                LambdaMARTParams::invalid("the validation dataset lives on device " + std::to_string(vdev->device_ordinal()) + ", the training dataset on device " +
                                          std::to_string(dev.device_ordinal()) + " (a validation dataset on another device is not supported)");
            stats_.valid_dataset = true;
            stats_.valid_dataset_queries = (uint32_t)vdev->nq(), stats_.valid_dataset_instances = (uint32_t)vdev->n();
        }
        struct ValidGuard {  // (the validation side holds nothing but its leaf cache beyond a call)
            frdev::DeviceDataset* d;
            bool dart;
            ~ValidGuard() {
                if (d && dart) d->dart_end();
            }
        } valid_guard{vdev, p_.dart()};

        Model out;
        out.kind = Model::Ensemble;
        // running scores: acc = 0, slot 0 = acc; with an init model acc = 0 + 1.0 * forest scores (exact), slot 0 = acc
        auto start_scores = [&](DatasetView& v, frdev::DeviceDataset& d) {
            if (!d.ensemble_begin(&err)) fail_str(err);
            if (T0 > 0) {
                score_model(v, *init_, &d);
                if (!d.ensemble_accumulate(1.0, &err)) fail_str(err);
            }
            if (!d.ensemble_finish(&err)) fail_str(err);
        };
        // the mean of the validation dataset's running scores over all of its queries, in its order
        auto valid_mean = [&]() {
            double m = 0.0;
            if (!vdev->metric_from_scores(vev_.measure, vev_.depth, vev_.norms.data(), 1, false, &err)) fail_str(err);
            if (!vdev->reduce_means(1, &m, &err)) fail_str(err);
            check_flags(*vdev);
            return m;
        };
        if (init_) {
            auto ti = tnow();
            out.members = init_->members, out.ens_weights = init_->ens_weights;
            start_scores(*view_, dev);
            if (vd) start_scores(*valid_, *vdev);
            if (!frdev::device_synchronize(&err)) fail_str(err);
            stats_.t_init = secs(ti, tnow());
            stats_.init_model = true, stats_.init_trees = T0;
        } else {
            start_scores(*view_, dev);
            if (vd) start_scores(*valid_, *vdev);
        }
        const char* rule = held_measure ? "---------------------------------------\n" : "-----------------------\n";
        if (!p_.quiet) {
            if (held_measure) printf("%s|%7s|%15s|%15s|\n%s", rule, "Tree", ev_.name.c_str(), "validation", rule);
            else printf("%s|%7s|%15s|\n%s", rule, "Tree", ev_.name.c_str(), rule);
        }
        std::vector<double> lam, wt, leaf_of(max_id + 1, 0.0);
        // per-tree samples: with both rates at 1.0 nothing below differs from a request without the keys
        // held-out queries: every tree's query list is a subset of T -- T itself, set once, without a query rate
        const bool sampling = p_.sampling(), sample_q = p_.query_sampling_rate < 1.0, sample_f = p_.feature_sampling_rate < 1.0;
        const bool subset_q = sample_q || hold, fixed_q = hold && !sample_q;
        Rand64 master(p_.seed);
        if (sampling)  // (an init model's trees have taken their seeds: two each)
            for (uint32_t i = 0; i < 2 * T0; i++) (void)master.rand_u64();
        std::vector<unsigned char> qflags;
        std::vector<uint32_t> t_ids, t_pos, t_feats, t_off;
        uint32_t t_n = 0;  // the tree's number of instances
        // the tree's query list -> flags, number of instances and (exact grower) instance list and positions
        auto take_queries = [&](const std::vector<uint32_t>& qs) {
            qflags.assign(csr.nq, 0);
            size_t n_t = 0;
            for (uint32_t q : qs) qflags[q] = 1, n_t += csr.qoff[q + 1] - csr.qoff[q];
            t_n = (uint32_t)n_t;
            if (hist) return;  // (the histogram grower makes its root list on the device from the flags)
            t_ids.clear(), t_pos.clear();
            for (uint32_t q : qs) {
                const size_t b = csr.qoff[q] - csr.qoff[0], e = csr.qoff[q + 1] - csr.qoff[0];
                t_ids.insert(t_ids.end(), root_ids.begin() + b, root_ids.begin() + e);
                t_pos.insert(t_pos.end(), positions.begin() + b, positions.begin() + e);
            }
            t_off = {0u, (uint32_t)t_ids.size()};
        };
        if (hold) {
            stats_.validation_queries = (uint32_t)split.held.size(), stats_.training_queries = (uint32_t)split.train.size();
            if (!dev.subset_means_set(split.train, split.held, &err)) fail_str(err);
            if (fixed_q) {
                take_queries(split.train);
                if (hist) hist->set_sample(qflags.data(), t_n, nullptr);
            }
        }
        // best_it: a tree count of the returned model (init trees included); 0 = no measure seen yet
        uint32_t trained = 0, best_it = 0;
        double best_valid = 0.0;
        if (init_) {  // the init model's own measures, from one metric pass: with a held-out measure it is the first best
            double mean = 0.0, two[2] = {0.0, 0.0};
            if (!dev.metric_from_scores(ev_.measure, ev_.depth, ev_.norms.data(), 1, false, &err)) fail_str(err);
            if (hold) {
                if (!dev.reduce_subset_means(two, &err)) fail_str(err);
                mean = two[0];
            } else if (!dev.reduce_means(1, &mean, &err)) {
                fail_str(err);
            }
            check_flags(dev);
            stats_.init_train_measure = mean;
            if (held_measure) {
                stats_.init_valid_measure = hold ? two[1] : valid_mean();
                if (T0 > 0) best_it = T0, best_valid = stats_.init_valid_measure;
            }
        }
        // DART: the drop plan, the leaf cache (one row per tree) and the weights so far; without drop_rate none of it exists
        const bool dart = p_.dart();
        DartPlan plan(p_.seed, p_.drop_rate, p_.max_drop, p_.skip_drop);
        Rand64 xe_keys(p_.seed ^ XENDCG_STREAM);  // the listwise objective's keys: a stream of its own, like the plan's
        GossKeys goss_keys(p_.seed);               // GOSS: one more stream of its own (lambdamart_goss.hpp)
        const bool goss = p_.goss();
        QuantKeys quant_keys(p_.seed);             // quantised gradients: and one more (lambdamart_quant.hpp)
        const bool quant = p_.grad_quant_bits != 0;
        for (uint32_t i = 0; i < T0; i++) {  // (an init model's trees have taken their keys: one each)
            if (p_.xendcg()) (void)xe_keys.rand_u64();
            if (goss) (void)goss_keys.next();
            if (quant) (void)quant_keys.next();
        }
        struct DartGuard {
            frdev::DeviceDataset& d;
            bool on;
            ~DartGuard() {
                if (on) d.dart_end();
            }
        } dart_guard{dev, dart};
        if (dart) {
            if (!dev.dart_begin(p_.num_trees, &stats_.dart_cache_bytes, &err)) fail_str(err);
            if (vd && !vdev->dart_begin(p_.num_trees, &stats_.valid_dart_cache_bytes, &err)) fail_str(err);
        }
        // the scores become sum_{i in trees} w_i tree_i(x), re-formed from tree 0 (slot 0 and the accumulator); waited for
        auto reform = [&](const std::vector<uint32_t>& trees) {
            auto t_a = tnow();
            if (!dev.dart_rescore(out.ens_weights.data(), out.ens_weights.size(), trees.data(), trees.size(), &err)) fail_str(err);
            if (!frdev::device_synchronize(&err)) fail_str(err);
            stats_.t_dart += secs(t_a, tnow());
        };
        for (uint32_t t = 0; t < p_.num_trees; t++) {
            const uint64_t xe_key = p_.xendcg() ? xe_keys.rand_u64() : 0;  // k_t: one per tree, before anything else of the tree
            const HistGoss goss_t{p_.goss_top_rate, p_.goss_other_rate, goss ? goss_keys.next() : 0};  // K_t: one per tree as well
            const uint64_t quant_key = quant ? quant_keys.next() : 0;
            const std::vector<uint32_t> dropped = dart ? plan.next(t) : std::vector<uint32_t>();
            if (!dropped.empty()) reform(dart_kept(t, dropped));  // the tree is fitted to the ensemble without the dropped trees
            auto ts = tnow();  // (drawing the sample and handing it to the grower count as grow time)
            LambdaSample smp;
            // the tree's instance list (a subsequence of the full one), feature list and positions
            const std::vector<uint32_t>*ids_t = &root_ids, *feats_t = &feats, *off_t = &root_off;
            const uint32_t* pos_t = positions.data();
            if (sampling) {
                smp = lambdamart_next_sample(master, feats.size(), csr.nq, p_, hold ? &split.train : nullptr);
                if (sample_q) take_queries(smp.queries);
                if (sample_f) {
                    t_feats.clear();
                    for (uint32_t s : smp.features) t_feats.push_back(feats[s]);
                    feats_t = &t_feats;
                }
                stats_.sum_queries += smp.queries.size(), stats_.sum_instances += subset_q ? t_n : root_ids.size(), stats_.sum_features += smp.features.size();
            }
            if (subset_q && !hist) ids_t = &t_ids, off_t = &t_off, pos_t = t_pos.data();
            auto ta = tnow();
            if (!dev.lambda_gradients(ev_.norms.data(), ev_.depth, p_.sigma, p_.pass(subset_q ? qflags.data() : nullptr, fixed_q && t > 0, xe_key), &err))
                fail_str(err);
            if (!frdev::device_synchronize(&err)) fail_str(err);
            auto tb = tnow();
            if (sampling && hist) {
                if (fixed_q) hist->set_sample(nullptr, t_n, sample_f ? &smp.features : nullptr, true);  // (T's root list stays)
                else hist->set_sample(sample_q ? qflags.data() : nullptr, t_n, sample_f ? &smp.features : nullptr);
            }
            HistTreeReport rep;
            std::shared_ptr<TreeNode> root = hist ? hist->grow(nullptr, nullptr, goss ? &goss_t : nullptr, &rep, quant_key)
                                                  : grower.grow_lambda_tree(dev, *off_t, *ids_t, *feats_t, pos_t, rst);
            auto tc = tnow() - std::chrono::duration_cast<std::chrono::steady_clock::duration>(std::chrono::duration<double>(rep.leaf_seconds));
            // leaves (exact grower): route every instance through a copy of the tree whose leaves hold their index
            std::vector<TreeNode*> leaves;
            std::shared_ptr<TreeNode> routing = hist ? nullptr : number_leaves(*root, leaves);
            if (!hist) {
                Model rm;
                rm.kind = Model::DecisionTree;
                rm.tree = routing;
                score_model(*view_, rm, &dev);
                if (!dev.download_scores(0, leaf_of.data(), leaf_of.size(), &err)) fail_str(err);
                if (!dev.lambda_download_positions(&lam, &wt, &err)) fail_str(err);
                std::vector<double> sl(leaves.size(), 0.0), sw(leaves.size(), 0.0);
                for (size_t g = 0; g < ids_t->size(); g++) {  // (the tree's instance list, in its order)
                    const double lv = leaf_of[(*ids_t)[g]];
                    if (!(lv >= 0.0 && lv < (double)leaves.size())) fail_str("LambdaMART: an instance was routed to no leaf");
                    const size_t L = (size_t)lv;
                    sl[L] = sl[L] + lam[pos_t[g]];
                    sw[L] = sw[L] + wt[pos_t[g]];
                }
                for (size_t L = 0; L < leaves.size(); L++) leaves[L]->value = sw[L] != 0.0 ? sl[L] / sw[L] : 0.0;
            }
            auto td = tnow();
            auto tu = td;  // where the update stage begins (DART: after the cache fill and the re-forming)
            Model tm;
            tm.kind = Model::DecisionTree;
            tm.tree = root;
            // DART: the tree's leaf values and the list of every tree so far, shared by the training and the validation side
            std::vector<double> values;
            std::vector<uint32_t> all;
            if (dart) {  // the tree's row of the leaf cache: the routing copy's scores (slot 0) are the documents' leaf numbers
                if (hist) {
                    Model rm;
                    rm.kind = Model::DecisionTree;
                    rm.tree = routing = number_leaves(*root, leaves);
                    score_model(*view_, rm, &dev);
                }
                values.resize(leaves.size());
                for (size_t L = 0; L < leaves.size(); L++) values[L] = leaves[L]->value;
                if (!dev.dart_fill(t, values.data(), values.size(), &err)) fail_str(err);
                if (!frdev::device_synchronize(&err)) fail_str(err);
                stats_.t_dart += secs(td, tnow());
                tu = tnow();
                dart_reweight(out.ens_weights, dropped, p_.learning_rate);
                stats_.dropped.push_back((uint32_t)dropped.size());
            } else {
                out.ens_weights.push_back(p_.learning_rate);
            }
            if (dart) {
                // the running scores under the new weights, from tree 0.  Without a drop that is acc + learning_rate * tree(x) bit
                // for bit, and streaming the cache is still the cheaper way to it (a single tree's walk costs several re-formings)
                all.resize(t + 1);
                for (uint32_t i = 0; i <= t; i++) all[i] = i;
                reform(all);
                tu = tnow();
            } else {
                // update: slot 0 = tree(x); acc = acc + learning_rate * slot 0; slot 0 = acc
                score_model(*view_, tm, &dev);
                if (!dev.ensemble_accumulate(p_.learning_rate, &err) || !dev.ensemble_finish(&err)) fail_str(err);
            }
            double mean = 0.0, two[2] = {0.0, 0.0};
            if (!dev.metric_from_scores(ev_.measure, ev_.depth, ev_.norms.data(), 1, false, &err)) fail_str(err);
            if (hold) {  // the means over T and H, from the one per-query pass
                if (!dev.reduce_subset_means(two, &err)) fail_str(err);
                mean = two[0];
            } else if (!dev.reduce_means(1, &mean, &err)) {
                fail_str(err);
            }
            check_flags(dev);
            auto te = tnow();
            // the validation dataset's side, a stage of its own: the same update on its own device form, then its plain mean
            double vmean = 0.0;
            if (vd) {
                if (dart) {
                    Model rm;
                    rm.kind = Model::DecisionTree;
                    rm.tree = routing;
                    score_model(*valid_, rm, vdev);
                    if (!vdev->dart_fill(t, values.data(), values.size(), &err)) fail_str(err);
                    if (!vdev->dart_rescore(out.ens_weights.data(), out.ens_weights.size(), all.data(), all.size(), &err)) fail_str(err);
                } else {
                    score_model(*valid_, tm, vdev);
                    if (!vdev->ensemble_accumulate(p_.learning_rate, &err) || !vdev->ensemble_finish(&err)) fail_str(err);
                }
                vmean = valid_mean();
                stats_.t_valid += secs(te, tnow());
            }
            stats_.t_gradient += secs(ta, tb);
            stats_.t_grow += secs(ts, ta) + secs(tb, tc);
            stats_.t_leaves += secs(tc, td);
            stats_.t_update += secs(tu, te);
            if (hist) stats_.sum_leaves += rep.leaves;
            if (hist) stats_.pool_bytes = hist->pool_bytes();
            if (hist && !signs.empty()) stats_.clamped_leaves.push_back(rep.clamped_leaves);
            if (goss) {
                stats_.t_goss += rep.goss_seconds;
                stats_.goss_instances.push_back(rep.goss_instances);
                stats_.goss_top.push_back(rep.goss_top);
            }
            if (quant) stats_.t_quant += rep.quant_seconds;
            if (hist && p_.symmetric_trees) stats_.levels.push_back(rep.levels);
            stats_.train_measure.push_back(mean);
            out.members.push_back(std::move(tm));
            if (!p_.quiet) {
                if (held_measure) printf("|%7u|%15.6f|%15.6f|\n", T0 + t + 1, mean, hold ? two[1] : vmean);
                else printf("|%7u|%15.6f|\n", T0 + t + 1, mean);
                fflush(stdout);
            }
            trained = t + 1;
            if (held_measure) {
                const double v = hold ? two[1] : vmean;
                const uint32_t iteration = T0 + trained;
                stats_.valid_measure.push_back(v);
                if (best_it == 0 || v > best_valid) best_it = iteration, best_valid = v;  // the FIRST maximum
                if (p_.early_stopping_rounds > 0 && iteration - best_it >= p_.early_stopping_rounds) {
                    stats_.stopped_early = trained < p_.num_trees;
                    break;
                }
            }
        }
        if (!p_.quiet) printf("%s", rule);
        stats_.trees = trained;
        stats_.best_iteration = best_it;
        stats_.best_valid_measure = best_valid;
        if (held_measure && p_.early_stopping_rounds > 0) {  // the ensemble up to the best tree (trees depend on their predecessors only)
            out.members.resize(best_it);
            out.ens_weights.resize(best_it);
        }
        stats_.seconds = secs(t0, tnow());
        return out;
    }

    const LambdaMARTStats& stats() const { return stats_; }

    // a copy of `n` whose leaves hold 0, 1, 2, ... in depth-first order; leaves[i] = the original leaf numbered i
    static std::shared_ptr<TreeNode> number_leaves(TreeNode& n, std::vector<TreeNode*>& leaves) {
        auto c = std::make_shared<TreeNode>();
        copy_numbered(n, *c, leaves);
        return c;
    }

  private:
    static void copy_numbered(TreeNode& n, TreeNode& c, std::vector<TreeNode*>& leaves) {
        c.leaf = n.leaf;
        c.fid = n.fid;
        if (n.leaf) {
            c.value = (double)leaves.size();
            leaves.push_back(&n);
            return;
        }
        c.value = n.value;
        c.lhs.reset(new TreeNode());
        c.rhs.reset(new TreeNode());
        copy_numbered(*n.lhs, *c.lhs, leaves);
        copy_numbered(*n.rhs, *c.rhs, leaves);
    }

    std::shared_ptr<DatasetView> view_, valid_;
    Evaluator ev_, vev_;
    const Model* init_ = nullptr;
    LambdaMARTParams p_;
    LambdaMARTStats stats_;
};

}  // namespace fr
