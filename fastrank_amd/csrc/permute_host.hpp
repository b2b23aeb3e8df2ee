// Host side of permutation importance (permute.hpp states the definition): the options and the
// refusals that need no device, the stream as a sort of (key, index) pairs, the conversion of instance ids to the positions
// the kernels address, which features a model reads at all, and the report.  No HIP, no environment.
#pragma once
#include <algorithm>
#include <cmath>
#include <memory>
#include <utility>
#include <vector>

#include "host.hpp"
#include "permute.hpp"

namespace fr {

struct PermuteOptions {
    uint32_t repeats = 5;
    uint64_t seed = 0;
    bool per_query = false;  // scope "query"
    bool has_features = false;
    std::vector<uint32_t> features;  // as given
    bool skip_unused = true;
    uint64_t max_slots = 0;  // 0: from free memory
};

inline bool permute_scope_from_string(const std::string& s) {
    if (s == "dataset") return false;
    if (s == "query") return true;
    fail_str("invalid value: scope must be \"dataset\" or \"query\", not \"" + s + "\"");
}

// {"repeats", "seed", "scope", "features", "skip_unused", "max_slots"}, each optional; any other key is refused by name
inline PermuteOptions permute_options_from_json(const Value& v) {
    if (!v.is_object()) fail_raw("Error(\"invalid type: expected a map for the permutation options\", line: 0, column: 0)");
    PermuteOptions o;
    for (const auto& kv : v.obj) {
        if (kv.first == "repeats") {
            const uint64_t r = json_u64(kv.second, "repeats");
            if (r < 1 || r > frpermute::MAX_REPEATS)
                fail_str("invalid value: repeats must be between 1 and " + std::to_string(frpermute::MAX_REPEATS) + ", not " + std::to_string(r));
            o.repeats = (uint32_t)r;
        } else if (kv.first == "seed") {
            o.seed = json_u64(kv.second, "seed");
        } else if (kv.first == "scope") {
            if (kv.second.kind != Value::String) fail_raw("Error(\"invalid type: expected a string for scope\", line: 0, column: 0)");
            o.per_query = permute_scope_from_string(kv.second.s);
        } else if (kv.first == "features") {
            if (!kv.second.is_array()) fail_raw("Error(\"invalid type: expected a sequence for features\", line: 0, column: 0)");
            o.has_features = true;
            for (const auto& f : kv.second.arr) o.features.push_back(json_u32(f, "features"));
        } else if (kv.first == "skip_unused") {
            o.skip_unused = json_bool(kv.second, "skip_unused");
        } else if (kv.first == "max_slots") {
            o.max_slots = json_u64(kv.second, "max_slots");
            if (o.max_slots < 1) fail_str("invalid value: max_slots must be at least 1");
        } else {
            fail_raw("Error(\"unknown field `" + kv.first +
                     "`, expected one of `repeats`, `seed`, `scope`, `features`, `skip_unused`, `max_slots`\", line: 0, column: 0)");
        }
    }
    return o;
}

// the features of the call in the order asked for (default: the view's, ascending); one the view does not hold, or one
// listed twice, is refused
inline std::vector<uint32_t> permute_features(const PermuteOptions& o, const std::vector<uint32_t>& view_features) {
    std::vector<uint32_t> have = view_features;
    std::sort(have.begin(), have.end());
    if (!o.has_features) return have;
    std::vector<uint32_t> seen;
    for (uint32_t f : o.features) {
        if (!std::binary_search(have.begin(), have.end(), f)) fail_str("invalid value: feature " + std::to_string(f) + " is not one of the dataset's features");
        if (std::find(seen.begin(), seen.end(), f) != seen.end()) fail_str("invalid value: feature " + std::to_string(f) + " is listed twice");
        seen.push_back(f);
    }
    return seen;
}

// what the kernels take
enum class PermuteShape { LINEAR, SINGLE, TREES, ENSEMBLE_LINEAR };

inline std::string permute_shape_name(const Model& m, int depth = 0) {
    switch (m.kind) {
        case Model::Linear: return "Linear";
        case Model::SingleFeature: return "SingleFeature";
        case Model::DecisionTree: return "DecisionTree";
        case Model::Ensemble: break;
    }
    std::string s = "Ensemble[";
    for (size_t k = 0; k < m.members.size(); k++) {
        if (k == 8 || depth > 2) {
            s += ", ...";
            break;
        }
        s += (k ? ", " : "") + permute_shape_name(m.members[k], depth + 1);
    }
    return s + "]";
}

inline PermuteShape permute_model_shape(const Model& m) {
    switch (m.kind) {
        case Model::Linear: return PermuteShape::LINEAR;
        case Model::SingleFeature: return PermuteShape::SINGLE;
        case Model::DecisionTree: return PermuteShape::TREES;
        case Model::Ensemble: break;
    }
    bool trees = !m.members.empty(), flat = !m.members.empty();
    for (const auto& mm : m.members) {
        trees = trees && mm.kind == Model::DecisionTree;
        flat = flat && (mm.kind == Model::Linear || mm.kind == Model::SingleFeature);
    }
    if (trees) return PermuteShape::TREES;
    if (flat) return PermuteShape::ENSEMBLE_LINEAR;
    fail_str("permutation importance takes a Linear, SingleFeature or DecisionTree model, an Ensemble of DecisionTrees or an Ensemble of Linear / "
             "SingleFeature models, not " + permute_shape_name(m));
}

// The model as the kernels take it (DeviceDataset::permute_score): its members in order, and what they point into.  Both
// stores keep their heap blocks when the record moves, so the members' pointers hold; it cannot be copied.
struct PermuteModel {
    std::vector<frdev::PermuteMember> members;
    std::vector<std::vector<double>> weights;  // the LINEAR members' weights over the matrix's d columns, in member order
    std::unique_ptr<frdev::FlatTrees> trees;   // the TREES member's forest
};

// `m` of shape `shape` for a matrix of d columns.  Linear weights past d are dropped and missing ones are 0.0; an Ensemble's
// zip(weights, models) stops at the shorter (src/model.rs:106).
inline PermuteModel permute_model(const Model& m, PermuteShape shape, size_t d) {
    PermuteModel pm;
    if (shape == PermuteShape::TREES) {
        pm.trees = std::make_unique<frdev::FlatTrees>();
        flat_trees_of(m, pm.trees.get());
        frdev::PermuteMember mem;
        mem.kind = frdev::PermuteMember::TREES, mem.trees = pm.trees.get();
        pm.members.push_back(mem);
        return pm;
    }
    auto add_flat = [&](const Model& mm, double ens_w) {
        frdev::PermuteMember mem;
        mem.ens_weight = ens_w;
        if (mm.kind == Model::Linear) {
            pm.weights.emplace_back(d, 0.0);
            for (size_t j = 0; j < d && j < mm.weights.size(); j++) pm.weights.back()[j] = mm.weights[j];
            mem.kind = frdev::PermuteMember::LINEAR;
        } else {
            mem.kind = frdev::PermuteMember::SINGLE, mem.fid = mm.fid, mem.dir = mm.dir;
        }
        pm.members.push_back(mem);
    };
    if (shape == PermuteShape::ENSEMBLE_LINEAR) {
        const size_t nt = std::min(m.members.size(), m.ens_weights.size());
        for (size_t t = 0; t < nt; t++) add_flat(m.members[t], m.ens_weights[t]);
    } else {
        add_flat(m, 1.0);
    }
    size_t k = 0;  // (the store no longer grows: its vectors' addresses hold)
    for (auto& mem : pm.members)
        if (mem.kind == frdev::PermuteMember::LINEAR) mem.weights = pm.weights[k++].data();
    return pm;
}

inline bool permute_tree_uses(const TreeNode& n, uint32_t f) {
    if (n.leaf) return false;
    return n.fid == f || permute_tree_uses(*n.lhs, f) || permute_tree_uses(*n.rhs, f);
}

// May the model's score change when column f changes?  colmax[f]: the column's largest |x| (+inf when it holds inf or NaN:
// 0 * inf is NaN, so a zero weight does not make such a column unused); f >= d reads 0.0 everywhere.
inline bool permute_feature_used(const Model& m, uint32_t f, const std::vector<double>& colmax) {
    switch (m.kind) {
        case Model::Linear:
            if (f >= colmax.size()) return false;
            return !(f >= m.weights.size() || m.weights[f] == 0.0) || !std::isfinite(colmax[f]);
        case Model::SingleFeature: return m.fid == f && f < colmax.size();
        case Model::DecisionTree: return f < colmax.size() && permute_tree_uses(*m.tree, f);
        case Model::Ensemble: {
            const size_t nt = std::min(m.members.size(), m.ens_weights.size());
            for (size_t k = 0; k < nt; k++)
                if (permute_feature_used(m.members[k], f, colmax)) return true;
            return false;
        }
    }
    return false;
}

// list indices 0 .. n-1 sorted by (key, index) ascending
inline void permute_sort(std::vector<std::pair<uint64_t, uint32_t>>& kv) { std::sort(kv.begin(), kv.end()); }

// src_index[i] = the list index whose value list index i reads in repeat r.  keys[i] = u_i; query_of[i] (scope "query"; null:
// scope "dataset") = any number that is equal for members of one query and different between queries.
inline void permute_sources_from_keys(const uint64_t* keys, const uint32_t* query_of, size_t n, uint32_t* src_index) {
    std::vector<std::pair<uint64_t, uint32_t>> kv(n);
    if (!query_of) {
        for (size_t i = 0; i < n; i++) kv[i] = {keys[i], (uint32_t)i};
        permute_sort(kv);
        for (size_t i = 0; i < n; i++) src_index[i] = kv[i].second;
        return;
    }
    // members of each query in ascending list index (a stable grouping), then each group sorted on its own
    std::vector<std::pair<uint32_t, uint32_t>> by_query(n);
    for (size_t i = 0; i < n; i++) by_query[i] = {query_of[i], (uint32_t)i};
    std::sort(by_query.begin(), by_query.end());
    for (size_t a = 0; a < n;) {
        size_t b = a;
        while (b < n && by_query[b].first == by_query[a].first) b++;
        for (size_t k = a; k < b; k++) kv[k] = {keys[by_query[k].second], by_query[k].second};
        std::sort(kv.begin() + a, kv.begin() + b);
        for (size_t k = a; k < b; k++) src_index[by_query[k].second] = kv[k].second;
        a = b;
    }
}

inline void permute_sources(uint64_t seed, uint32_t r, const uint32_t* query_of, size_t n, uint32_t* src_index) {
    const uint64_t key_r = frpermute::repeat_key(frpermute::stream_key(seed), r);
    std::vector<uint64_t> keys(n);
    for (size_t i = 0; i < n; i++) keys[i] = frpermute::element_key(key_r, i);
    permute_sources_from_keys(keys.data(), query_of, n, src_index);
}

// The kernels address padded positions: instance_at[p] = the instance id at position p (0xFFFFFFFF: none).  ids[n] = I,
// ascending.  Returns pos[i] = the position of ids[i] (the inverse of instance_at over the view).  An id of I that has no
// position is refused (the device form does not hold the view).
inline std::vector<uint32_t> permute_position_table(const uint32_t* instance_at, size_t np, const uint32_t* ids, size_t n) {
    std::vector<std::pair<uint32_t, uint32_t>> pos_of;  // (id, position), sorted by id
    pos_of.reserve(n);
    for (size_t p = 0; p < np; p++)
        if (instance_at[p] != 0xFFFFFFFFu) pos_of.emplace_back(instance_at[p], (uint32_t)p);
    std::sort(pos_of.begin(), pos_of.end());
    if (pos_of.size() != n) fail_str("permutation importance: the device form holds " + std::to_string(pos_of.size()) + " documents, the view " + std::to_string(n));
    std::vector<uint32_t> pos(n);
    for (size_t i = 0; i < n; i++) {
        if (pos_of[i].first != ids[i]) fail_str("permutation importance: instance " + std::to_string(ids[i]) + " has no position on the device");
        pos[i] = pos_of[i].second;
    }
    return pos;
}

// out[p] = the position whose value position p reads: pos[src_index[i]] at pos[i], p itself wherever no document of the view sits
inline void permute_positions(const uint32_t* pos, const uint32_t* src_index, size_t n, size_t np, uint32_t* out) {
    for (size_t p = 0; p < np; p++) out[p] = (uint32_t)p;
    for (size_t i = 0; i < n; i++) out[pos[i]] = pos[src_index[i]];
}

struct PermuteScore {
    double importance = 0.0, std = 0.0;
};

// d_r = baseline - values[r]; importance = (sum_r d_r in order) / R; std = sqrt(sum_r (d_r - importance)^2 / (R - 1)), 0.0 at R = 1
inline PermuteScore permute_report(double baseline, const double* values, size_t R) {
    PermuteScore s;
    double sum = 0.0;
    for (size_t r = 0; r < R; r++) {
        const double d = baseline - values[r];
        sum = sum + d;
    }
    s.importance = sum / (double)R;
    if (R > 1) {
        double ss = 0.0;
        for (size_t r = 0; r < R; r++) {
            const double d = baseline - values[r];
            const double e = d - s.importance;
            const double sq = e * e;
            ss = ss + sq;
        }
        s.std = std::sqrt(ss / (double)(R - 1));
    }
    return s;
}

}  // namespace fr
