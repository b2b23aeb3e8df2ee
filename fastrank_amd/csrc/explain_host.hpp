// Host side of the model explanation: which models can be explained, the trees as the cover pass
// walks them, and the path table explain.hip's kernel reads, built from the trees and the background's leaf counts.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <map>

#include "explain.hpp"
#include "host.hpp"

namespace fr {

struct ExplainModel {
    std::vector<const TreeNode*> trees;
    std::vector<double> weights;
    std::vector<uint32_t> feats;         // the features some tree splits on, ascending
    std::vector<uint64_t> split_counts;  // ... and how many split nodes each has, over all trees
};

inline void explain_check_tree(const TreeNode& n, std::map<uint32_t, uint64_t>& splits) {
    if (!std::isfinite(n.value)) fail_str("explain: the model holds a leaf value or a split that is not finite");
    if (n.leaf) return;
    splits[n.fid]++;
    explain_check_tree(*n.lhs, splits);
    explain_check_tree(*n.rhs, splits);
}

// A DecisionTree, or an Ensemble of DecisionTrees (zip(weights, models) stops at the shorter: src/model.rs:106).
inline ExplainModel explain_model(const Model& m) {
    ExplainModel out;
    switch (m.kind) {
        case Model::Linear: fail_str("explain: a Linear model has no trees to explain (its contributions are weight * value)");
        case Model::SingleFeature: fail_str("explain: a SingleFeature model has no trees to explain");
        case Model::DecisionTree:
            out.trees.push_back(m.tree.get());
            out.weights.push_back(1.0);
            break;
        case Model::Ensemble: {
            const size_t nt = std::min(m.members.size(), m.ens_weights.size());
            for (const Model& mm : m.members) {
                if (mm.kind == Model::Ensemble) fail_str("explain: nested ensembles are not supported, only an Ensemble of DecisionTrees");
                if (mm.kind != Model::DecisionTree) fail_str("explain: every member of the Ensemble must be a DecisionTree");
            }
            for (size_t t = 0; t < nt; t++) {
                out.trees.push_back(m.members[t].tree.get());
                out.weights.push_back(m.ens_weights[t]);
            }
            break;
        }
    }
    std::map<uint32_t, uint64_t> splits;
    for (const TreeNode* t : out.trees) explain_check_tree(*t, splits);
    for (double w : out.weights)
        if (!std::isfinite(w)) fail_str("explain: the model holds a weight that is not finite");
    for (const auto& kv : splits) out.feats.push_back(kv.first), out.split_counts.push_back(kv.second);
    return out;
}

inline int32_t explain_walk_tree(const TreeNode& n, frdev::ExWalk& w, uint32_t& next_leaf) {
    const int32_t idx = (int32_t)w.fid.size();
    w.fid.push_back(-1), w.lhs.push_back(-1), w.rhs.push_back(-1), w.split.push_back(n.value);
    if (n.leaf) {
        w.lhs[idx] = (int32_t)next_leaf++;
    } else {
        if (n.fid > (uint32_t)std::numeric_limits<int32_t>::max()) fail_str("explain: feature id " + std::to_string(n.fid) + " is too large");
        w.fid[idx] = (int32_t)n.fid;
        const int32_t l = explain_walk_tree(*n.lhs, w, next_leaf);
        const int32_t r = explain_walk_tree(*n.rhs, w, next_leaf);
        w.lhs[idx] = l, w.rhs[idx] = r;
    }
    return idx;
}

inline frdev::ExWalk explain_walk(const ExplainModel& em) {
    frdev::ExWalk w;
    uint32_t next_leaf = 0;
    w.leaf0.push_back(0);
    for (const TreeNode* t : em.trees) {
        w.root.push_back(explain_walk_tree(*t, w, next_leaf));
        w.leaf0.push_back(next_leaf);
    }
    return w;
}

struct ExplainPlan {
    frdev::ExTables tab;
    double bias = 0.0;  // sum over the trees, ascending, of w_t * v_t(no feature known)
};

struct ExplainPathBuilder {
    struct Elem {
        uint32_t slot;
        double lo, hi, z;
    };
    const std::vector<uint32_t>& counts;
    frdev::ExTables& tab;
    uint32_t dataset_d;
    const std::vector<uint32_t>& model_feats;
    std::vector<Elem> path;
    std::vector<uint32_t> tree_feats;  // slot -> feature id, in order of first occurrence
    uint32_t next_leaf = 0;

    // documents of the background under the node, leaves counted depth first from `leaf`
    uint64_t cover(const TreeNode& n, uint32_t& leaf) const {
        if (n.leaf) return counts[leaf++];
        const uint64_t l = cover(*n.lhs, leaf);
        return l + cover(*n.rhs, leaf);
    }
    uint32_t slot_of(uint32_t fid) {
        for (uint32_t s = 0; s < tree_feats.size(); s++)
            if (tree_feats[s] == fid) return s;
        tree_feats.push_back(fid);
        return (uint32_t)tree_feats.size() - 1;
    }
    // returns v(node): the value with no feature known
    double node(const TreeNode& n) {
        if (n.leaf) {
            tab.m.push_back((uint32_t)path.size());
            tab.eoff.push_back((uint32_t)tab.slot.size());
            tab.value.push_back(n.value);
            for (const Elem& e : path) tab.slot.push_back(e.slot), tab.lo.push_back(e.lo), tab.hi.push_back(e.hi), tab.z.push_back(e.z);
            tab.max_path = std::max<uint32_t>(tab.max_path, (uint32_t)path.size());
            next_leaf++;
            return n.value;
        }
        uint32_t probe = next_leaf;
        const uint64_t cl = cover(*n.lhs, probe), cr = cover(*n.rhs, probe), cp = cl + cr;
        const double rl = cp ? (double)cl / (double)cp : 0.0, rr = cp ? (double)cr / (double)cp : 0.0;
        const uint32_t slot = slot_of(n.fid);
        size_t at = 0;
        while (at < path.size() && path[at].slot != slot) at++;
        const bool fresh = at == path.size();
        if (fresh) {
            if (path.size() >= frdev::EX_MAX_PATH)
                fail_str("explain: a root-to-leaf path with more than " + std::to_string(frdev::EX_MAX_PATH) +
                         " distinct features is longer than the explain kernel supports (" + std::to_string(frdev::EX_MAX_PATH) + ")");
            path.push_back(Elem{slot, -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity(), 1.0});
        }
        const Elem saved = path[at];
        path[at].hi = std::min(saved.hi, n.value);
        path[at].z = saved.z * rl;
        const double vl = node(*n.lhs);
        path[at] = saved;
        path[at].lo = std::max(saved.lo, n.value);
        path[at].z = saved.z * rr;
        const double vr = node(*n.rhs);
        if (fresh) path.pop_back();
        else path[at] = saved;
        const double a = rl * vl, b = rr * vr;
        return a + b;
    }
};

// leaf_counts[L]: documents of the background at leaf L (explain_walk's numbering); dataset_d: features the explained
// dataset's matrix holds (a feature beyond it reads 0.0)
inline ExplainPlan explain_plan(const ExplainModel& em, const std::vector<uint32_t>& leaf_counts, uint32_t dataset_d) {
    ExplainPlan plan;
    frdev::ExTables& tab = plan.tab;
    tab.ncols = (uint32_t)em.feats.size();
    tab.leaf0.push_back(0), tab.feat0.push_back(0);
    ExplainPathBuilder b{leaf_counts, tab, dataset_d, em.feats};
    for (size_t t = 0; t < em.trees.size(); t++) {
        b.tree_feats.clear();
        b.path.clear();
        const double v = b.node(*em.trees[t]);
        const double prod = em.weights[t] * v;
        plan.bias = plan.bias + prod;
        tab.weight.push_back(em.weights[t]);
        for (uint32_t fid : b.tree_feats) {
            tab.fid.push_back(fid < dataset_d ? fid : frdev::EX_NO_FEATURE);
            tab.col.push_back((uint32_t)(std::lower_bound(em.feats.begin(), em.feats.end(), fid) - em.feats.begin()));
        }
        tab.max_tree_feats = std::max<uint32_t>(tab.max_tree_feats, (uint32_t)b.tree_feats.size());
        tab.leaf0.push_back(b.next_leaf);
        tab.feat0.push_back((uint32_t)tab.fid.size());
    }
    return plan;
}

}  // namespace fr
