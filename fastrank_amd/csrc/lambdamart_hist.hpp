// LambdaMART's histogram grower, host side ("Histogram grower"; device side: kernels_hist.inc).
//
// The tree is grown level by level.  The device holds the u8 bin matrix (built once per instance list, feature list and k),
// the tree's int64 fixed-point gradients Q / W, an index list partitioned by node and the level's histograms; the host
// holds the tree and applies the selection rule: per node the largest importance over the features' last-maximum
// candidates, the later feature among equals.  A level's histograms are built for the smaller child of every split and
// derived for the larger one (parent - child: integer sums, so exact).  Leaf values come from the leaves' own integer sums:
// the partition a split trains on (bins 0..j) is the one the scoring rule applies (x <= edge_j), so no routing pass.
// split_gain = "newton" ("Newton split gain"): the histograms also carry sum W, a candidate's
// importance is term(L) + term(R) with term = G G / (H + lambda_l2), a node splits only when that exceeds its own term by
// more than min_split_gain, and leaves are G / (H + lambda_l2).
// max_leaves >= 2 ("Leaf-wise growth"): the tree is grown one leaf at a time instead, always the open
// leaf whose best split gains most, until it has max_leaves leaves; the device keeps a pool of histograms, one per open
// leaf, and returns one record per searched node (grow_leaves below).  max_leaves = 0 is the level loop, untouched.
// monotone constraints ("Monotone constraints"; Newton gain only): some feature carries a sign, every
// node an interval [lo, hi] for its output; the device's candidates are those of the monotone scan kernels, and the host
// derives the children's intervals from the winning record's integer sums by the same two-case rule (monotone_term below).
// Without a non-zero sign nothing here differs.
// GOSS ("GOSS"; lambdamart_goss.hpp, kernels_goss.inc; Newton gain only): grow() is handed the two
// rates and the tree's key; the device cuts the sample's list down to the top set and a Bernoulli sample of the others, and
// the tree is grown over that list (n_ is then its length) from amplified gradients.  Without the argument nothing differs.
// symmetric trees ("Symmetric trees"; level-wise, no monotone signs): a level's open nodes all split on
// one candidate, the last maximum of the level importance (hist_scan_sym_kernel: one record per feature); a second launch
// (hist_sym_apply_kernel) returns every node's own record under that winner, and the level loop goes on as ever: a node that
// does not split under the winner closes into a leaf.  Without the option the loop launches what it launched before.
// leaf regularisation ("Leaf regularisation"; lambdamart_reg.hpp, kernels_histreg.inc; Newton gain only):
// lambda_l1, max_delta_step, path_smooth move a node's output off G / (H + lambda_l2); every node then carries its output next to
// its interval, the device's candidates are those of the regularised scan kernels (with or without monotone signs), and the
// host prices a node's own term, the children's outputs and intervals and the leaves by lambdamart_reg.hpp.  With all three at
// 0 nothing here differs.
// quantised gradients ("Quantised gradients"; lambdamart_quant.hpp, kernels_histquant.inc; Newton gain
// only, without monotone signs or leaf regularisation): grow() is handed the tree's key; after the fixed-point step the device
// rounds every entry's (Q, W) stochastically to quant_bits bits, and the tree carries two exponent pairs: the search's
// (how_.s_l / s_w = S - d, S_w - d_w: every sum a search returns is one of the small integers) and the leaves' (leaf_s_l_ /
// leaf_s_w_ = S, S_w: the leaf sums are still those of Q and W).  With quant_bits = 0 the two pairs are equal and nothing differs.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>

#include "host.hpp"
#include "lambdamart_goss.hpp"
#include "lambdamart_quant.hpp"
#include "lambdamart_reg.hpp"

namespace fr {

// the Newton gain's numbers (on = false: the variance criterion, and none of them is read)
struct HistNewton {
    bool on = false;
    double lambda_l2 = 0.0, min_sum_hessian = 0.0, min_split_gain = 0.0;
};

// GOSS for one tree: the two rates and the tree's key K_t
struct HistGoss {
    double top_rate = 0.0, other_rate = 0.1;
    uint64_t key = 0;
};

// what a grower is made with: k = split_candidates (bins per feature), the depth limit, the least leaf support, the split
// criterion, the leaf budget (0: level-wise growth) and the monotone signs: one of {-1, 0, +1} per entry of the ascending
// feature list (empty, or all 0: no constraint; a non-zero one needs the Newton gain)
struct HistGrowOptions {
    uint32_t k = 0, max_depth = 0, min_leaf = 0;
    HistNewton newton;
    uint32_t max_leaves = 0;
    std::vector<int> monotone;
    bool symmetric = false;
    HistReg reg;  // leaf regularisation (all 0: off; a non-zero one needs the Newton gain)
    uint32_t quant_bits = 0;  // quantised gradients (0: off; 2..8 need the Newton gain, no monotone sign and no leaf regularisation)
};

// what grow() reports of the tree it made, next to the tree
struct HistTreeReport {
    uint32_t leaves = 1;
    double leaf_seconds = 0.0;    // the share of the leaf sums
    uint32_t clamped_leaves = 0;  // monotone constraints: the leaves whose value a bound moved
    uint32_t levels = 0;          // symmetric trees: the levels that split (the tree's depth in splits)
    // GOSS: the list's length, the top set's size, tau and the wall seconds of making the list
    uint32_t goss_instances = 0, goss_top = 0;
    uint64_t goss_tau = 0;
    double goss_seconds = 0.0;
    double quant_seconds = 0.0;  // quantised gradients: the wall seconds of the quantise launch
};

class HistGrower {
    using Dev = frdev::DeviceDataset;

  public:
    HistGrower(Dev& dev, std::vector<uint32_t> feats, const HistGrowOptions& opt)
        : dev_(dev), feats_(std::move(feats)), k_(opt.k), max_depth_(opt.max_depth), min_leaf_(opt.min_leaf), newton_(opt.newton), max_leaves_(opt.max_leaves), symmetric_(opt.symmetric), reg_(opt.reg), reg_on_(opt.reg.on()), quant_bits_(opt.quant_bits) {
        for (int c : opt.monotone) mono_on_ = mono_on_ || c != 0;
        if (symmetric_ && max_leaves_ != 0) fail_str("LambdaMART histogram grower: symmetric trees are grown level by level (max_leaves must be 0)");
        if (symmetric_ && mono_on_) fail_str("LambdaMART histogram grower: symmetric trees take no monotone constraints");
        if (mono_on_) {
            if (!newton_.on) fail_str("LambdaMART histogram grower: monotone constraints need the Newton gain");
            if (opt.monotone.size() != feats_.size()) fail_str("LambdaMART histogram grower: one monotone sign per feature is needed");
            mono_ = opt.monotone;
        }
        if (reg_on_) {
            if (!newton_.on) fail_str("LambdaMART histogram grower: lambda_l1, max_delta_step and path_smooth need the Newton gain");
            if (symmetric_ && reg_.path_smooth != 0.0) fail_str("LambdaMART histogram grower: symmetric trees take no path_smooth");
            if (!mono_on_) mono_.assign(feats_.size(), 0);  // (the regularised scan kernels read a sign per feature)
        }
        if (quant_bits_ != 0) {
            if (!quant_bits_ok(quant_bits_)) fail_str("LambdaMART histogram grower: grad_quant_bits must be 0 or between 2 and 8");
            if (!newton_.on) fail_str("LambdaMART histogram grower: quantised gradients need the Newton gain");
            if (mono_on_ || reg_on_)
                fail_str("LambdaMART histogram grower: quantised gradients take no monotone constraints, lambda_l1, max_delta_step or path_smooth");
        }
    }
    ~HistGrower() { dev_.hist_end(); }

    // bins for the instance list at `positions`; true when they were built now (false: the view's kept ones were reused)
    bool prepare(const std::vector<uint32_t>& positions) {
        std::string err;
        bool built = false;
        if (!dev_.hist_bins(positions.data(), positions.size(), feats_, k_, &built, &err)) fail_str(err);
        if (!dev_.hist_edges(&edges_, &nedges_, &err)) fail_str(err);
        if ((mono_on_ || reg_on_) && !dev_.hist_monotone(mono_.data(), mono_.size(), &err)) fail_str(err);
        n_ = n_sample_ = n_full_ = (uint32_t)positions.size();
        sel_.clear();
        return built;
    }

    // The sample of the trees grown from now on ("Sampling").  query_flags[q] != 0: query q of the
    // view is in the sample, n_t of the instance list's entries in all (nullptr: every query); features: ascending indices
    // into the feature list (nullptr: every feature).  Bins and edges stay those of the full lists.
    // keep_queries (query_flags == nullptr): the query sample set before stays, e.g. a fixed training split under per-tree
    // feature samples.
    void set_sample(const unsigned char* query_flags, uint32_t n_t, const std::vector<uint32_t>* features, bool keep_queries = false) {
        std::string err;
        if (keep_queries && !query_flags) {
            if (features) sel_ = *features;
            else sel_.clear();
            check_features(features);
            if (!dev_.hist_sample(nullptr, n_sample_, features ? sel_.data() : nullptr, sel_.size(), &err, true)) fail_str(err);
            return;
        }
        if (features) sel_ = *features;
        else sel_.clear();
        check_features(features);
        if (!dev_.hist_sample(query_flags, query_flags ? n_t : n_full_, features ? sel_.data() : nullptr, sel_.size(), &err)) fail_str(err);
        n_ = n_sample_ = query_flags ? n_t : n_full_;
    }

    // One tree for the gradients of the last gradient pass (lam_list == nullptr) or for lam_list / wt_list[n] in
    // instance-list order.  goss (nullptr: none; Newton gain only): the tree is fitted to the GOSS list of the sample's list.
    // *report (may be nullptr): what else the tree left behind.  quant_key: the tree's key under quantised gradients (read only
    // when the grower was made with quant_bits != 0).
    // The calls a tree makes, in order: hist_goss (GOSS only), hist_quantise, hist_quantq (quantised gradients only); level-wise hist_root, then per level
    // hist_search (symmetric trees: hist_search_symmetric and hist_symmetric_apply) and hist_split; leaf-wise
    // hist_leaf_begin, then one hist_leaf_step per split; at the end hist_leaf_sums (after hist_root, when nothing was searched).
    std::shared_ptr<TreeNode> grow(const double* lam_list, const double* wt_list, const HistGoss* goss = nullptr, HistTreeReport* report = nullptr,
                                   uint64_t quant_key = 0) {
        std::string err;
        HistTreeReport rep;
        bool all_zero = false;
        n_ = n_sample_;
        if (goss != nullptr) {
            if (!newton_.on) fail_str("LambdaMART histogram grower: GOSS needs the Newton gain");
            auto t0 = std::chrono::steady_clock::now();
            const GossPlan plan = goss_plan(n_sample_, goss->top_rate, goss->other_rate);
            if (!dev_.hist_goss(lam_list, plan.n_top, plan.p, plan.amp, goss->key, &rep.goss_instances, &rep.goss_tau, &err)) fail_str(err);
            rep.goss_top = plan.n_top;
            n_ = rep.goss_instances;
            rep.goss_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        how_ = {min_leaf_, newton_.on, 0, 0, newton_.lambda_l2, newton_.min_sum_hessian, newton_.min_split_gain, mono_on_,
                reg_.lambda_l1, reg_.max_delta_step, reg_.path_smooth};
        if (!dev_.hist_quantise(lam_list, wt_list, &how_.s_l, &how_.s_w, &all_zero, &err)) fail_str(err);
        leaf_s_l_ = how_.s_l, leaf_s_w_ = how_.s_w;
        auto root = std::make_shared<TreeNode>();
        if (!all_zero) {  // (else one leaf of value 0.0)
            if (quant_bits_ != 0) {  // the searches read sums of (1, q, w) under (S - d, S_w - d_w); the leaves stay with Q / W
                auto t0 = std::chrono::steady_clock::now();
                int d = 0, d_w = 0;
                if (!dev_.hist_quantq(quant_bits_, quant_key, &d, &d_w, &err)) fail_str(err);
                how_.s_l -= d, how_.s_w -= d_w;
                rep.quant_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            }
            Leaves lv;
            const bool rooted = max_leaves_ >= 2 ? grow_leaves(root.get(), &lv) : grow_levels(root.get(), &lv, &rep.levels);
            rep.leaves = (uint32_t)lv.nodes.size();
            leaf_values(lv, rooted, &rep);
        }
        if (report) *report = rep;
        return root;
    }

    // leaf-wise growth: the largest histogram pool a tree of this grower asked for, in bytes (0: none yet)
    uint64_t pool_bytes() const { return pool_bytes_; }

  private:
    // A node that may still split.  Leaf-wise growth also keeps its creation index and the record and gain it is open with.
    struct Open {
        TreeNode* node;
        uint32_t slot, begin, end, depth;
        Dev::HistBounds bd;  // (read only under monotone constraints and leaf regularisation)
        uint32_t index = 0;
        double gain = 0.0;
        Dev::HistCand pick = {};
        // leaf regularisation: the node's parent's output (has_parent = false: the root) and its own, set by may_split
        double parent_out = 0.0;
        bool has_parent = false;
        double out = 0.0;
    };
    // the tree's leaves in the order they were closed: node, stretch of the index list (slot: its number), interval, and
    // (leaf regularisation) its parent's output
    struct Leaves {
        std::vector<TreeNode*> nodes;
        std::vector<Dev::HistNode> stretches;
        std::vector<Dev::HistBounds> bounds;
        std::vector<double> parent_out;
        std::vector<unsigned char> has_parent;
        void close(TreeNode* t, uint32_t b, uint32_t e, const Dev::HistBounds& bd, double parent = 0.0, bool with_parent = false) {
            nodes.push_back(t);
            stretches.push_back({(uint32_t)stretches.size(), b, e});
            bounds.push_back(bd);
            parent_out.push_back(parent);
            has_parent.push_back(with_parent ? 1 : 0);
        }
        void close(const Open& o) { close(o.node, o.begin, o.end, o.bd, o.parent_out, o.has_parent); }
    };

    // Level-wise growth.  false: the root was not searched, and the device's index list was not made.
    bool grow_levels(TreeNode* root, Leaves* lv, uint32_t* levels) {
        std::string err;
        if (!enterable(n_, 1)) {
            lv->close(root, 0u, n_, whole_line());
            return false;
        }
        if (!dev_.hist_root(newton_.on, &err)) fail_str(err);
        std::vector<Open> open{{root, 0u, 0u, n_, 1u, whole_line()}}, next;
        const size_t F = features();
        std::vector<Dev::HistNode> nodes, builds;
        std::vector<Dev::HistBounds> node_bounds;
        std::vector<Dev::HistRegNode> node_regs;
        std::vector<Dev::HistCand> best;
        std::vector<Dev::HistSymBest> level;
        std::vector<Dev::HistSplit> splits;
        std::vector<Dev::HistSub> subs;
        while (!open.empty()) {
            nodes.clear(), builds.clear(), splits.clear(), subs.clear(), next.clear(), node_bounds.clear(), node_regs.clear();
            for (const Open& o : open) nodes.push_back({o.slot, o.begin, o.end});
            size_t sym_f = 0;  // (symmetric trees) the level's winning feature; best[a]: node a's record under the winner
            if (symmetric_) {
                if (!dev_.hist_search_symmetric(nodes, how_, &level, &err)) fail_str(err);
                const Dev::HistSymBest* lw = nullptr;
                for (size_t fi = 0; fi < F; fi++)  // the last maximum: a later feature wins among equals
                    if (level[fi].valid && (lw == nullptr || level[fi].key >= lw->key)) lw = &level[fi], sym_f = fi;
                best.assign(open.size(), Dev::HistCand{});
                if (lw != nullptr) {
                    if (!dev_.hist_symmetric_apply(nodes, how_, (uint32_t)sym_f, lw->edge, &best, &err)) fail_str(err);
                    bool some = false;
                    for (const Dev::HistCand& b : best) some = some || b.valid;
                    if (!some) fail_str("LambdaMART histogram grower: internal error: no node splits under the level's winner");
                    (*levels)++;
                }
            } else {
                if (reg_on_)
                    for (const Open& o : open) node_regs.push_back({o.bd.lo, o.bd.hi, o.parent_out, o.has_parent ? 1u : 0u, 0u});
                else if (mono_on_)
                    for (const Open& o : open) node_bounds.push_back(o.bd);
                if (!dev_.hist_search(nodes, how_, mono_on_ && !reg_on_ ? &node_bounds : nullptr, &best, &err, reg_on_ ? &node_regs : nullptr))
                    fail_str(err);
            }
            uint32_t next_slots = 0;
            for (size_t a = 0; a < open.size(); a++) {
                Open& o = open[a];
                const uint32_t n = o.end - o.begin;
                const Dev::HistCand* w = nullptr;
                size_t wf = 0;
                if (symmetric_) {  // (the record's valid already holds the whole rule, the Newton gain's floor included)
                    if (best[a].valid) w = &best[a], wf = sym_f;
                } else {
                    for (size_t fi = 0; fi < F; fi++) {  // the last maximum: a later feature wins among equals
                        const Dev::HistCand& b = best[a * F + fi];
                        if (b.valid && (w == nullptr || b.imp >= w->imp)) w = &b, wf = fi;
                    }
                    double gain = 0.0;  // the node's totals (Qnode, Wnode) arrive with every record of the node
                    if (w != nullptr && !may_split(*w, n, &o, &gain)) w = nullptr;
                }
                if (w == nullptr) {
                    lv->close(o);
                    continue;
                }
                if (symmetric_ && reg_on_) o.out = node_output(*w, n, o);  // (may_split was not asked)
                Dev::HistBounds bl = o.bd, br = o.bd;
                if (mono_on_) child_bounds(o, n, mono_[full(wf)], *w, &bl, &br);
                const uint32_t nl = w->nl, nr = n - nl;
                const size_t ws = split_node(o.node, wf, w->edge, n, nl);
                splits.push_back({o.begin, o.end, (uint32_t)ws, w->edge, nl});  // (the bin matrix's row)
                const uint32_t mid = o.begin + nl;
                const bool el = enterable(nl, o.depth + 1), er = enterable(nr, o.depth + 1);
                if (!el) lv->close(o.node->lhs.get(), o.begin, mid, bl, o.out, true);
                if (!er) lv->close(o.node->rhs.get(), mid, o.end, br, o.out, true);
                if (!el && !er) continue;
                const bool left_small = nl <= nr;
                const uint32_t small_slot = next_slots++;
                builds.push_back(left_small ? Dev::HistNode{small_slot, o.begin, mid} : Dev::HistNode{small_slot, mid, o.end});
                uint32_t large_slot = 0;
                if (left_small ? er : el) {
                    large_slot = next_slots++;
                    subs.push_back({o.slot, small_slot, large_slot});
                }
                if (el) next.push_back({o.node->lhs.get(), left_small ? small_slot : large_slot, o.begin, mid, o.depth + 1, bl, 0u, 0.0, {}, o.out, true});
                if (er) next.push_back({o.node->rhs.get(), left_small ? large_slot : small_slot, mid, o.end, o.depth + 1, br, 0u, 0.0, {}, o.out, true});
            }
            if (!dev_.hist_split(splits, builds, subs, next_slots, newton_.on, &err)) fail_str(err);
            open.swap(next);
        }
        return true;
    }

    // Leaf-wise growth.  Every node has a creation index (the root 0; a split gives its lhs the next one, then its rhs); a
    // leaf that is enterable is searched when it is made and is open when its record is accepted by the level loop's rule;
    // the open leaf with the largest gain is split (the smallest creation index among equals) while the tree has fewer than
    // max_leaves leaves.  Fills *lv like the level loop does.  false: the root was not searched, and the device's index list
    // was not made.
    bool grow_leaves(TreeNode* root, Leaves* lv) {
        std::string err;
        std::vector<Open> open;
        if (!enterable(n_, 1)) {
            lv->close(root, 0u, n_, whole_line());
            return false;
        }
        // live histograms never exceed the leaves, and the leaves neither max_leaves, the instances nor 2^(max_depth - 1)
        uint32_t slots = std::min(max_leaves_, n_);
        if (max_depth_ <= 31) slots = std::min(slots, 1u << (max_depth_ - 1));
        std::vector<uint32_t> free_slots;
        for (uint32_t s = slots; s-- > 1;) free_slots.push_back(s);  // (slot 0: the root's)
        // a searched leaf with its record: open with its gain, or closed and its slot free again
        auto consider = [&](Open o) {
            if (may_split(o.pick, o.end - o.begin, &o, &o.gain)) {
                open.push_back(o);
            } else {
                lv->close(o);
                free_slots.push_back(o.slot);
            }
        };
        Dev::HistCand pick[2];
        if (!dev_.hist_leaf_begin(slots, how_, &pick[0], &err)) fail_str(err);
        consider({root, 0u, 0u, n_, 1u, whole_line(), 0u, 0.0, pick[0]});
        uint32_t n_leaves = 1, next_index = 1;
        while (n_leaves < max_leaves_ && !open.empty()) {
            size_t at = 0;
            for (size_t i = 1; i < open.size(); i++)
                if (open[i].gain > open[at].gain || (open[i].gain == open[at].gain && open[i].index < open[at].index)) at = i;
            const Open o = open[at];
            open.erase(open.begin() + (std::ptrdiff_t)at);
            const uint32_t n = o.end - o.begin, nl = o.pick.nl, nr = n - nl;
            const size_t ws = split_node(o.node, o.pick.fi, o.pick.edge, n, nl);
            n_leaves++;
            const uint32_t mid = o.begin + nl, il = next_index++, ir = next_index++;
            const bool more = n_leaves < max_leaves_;  // (the split that reaches max_leaves searches no child)
            const bool el = more && enterable(nl, o.depth + 1), er = more && enterable(nr, o.depth + 1);
            const bool left_small = nl <= nr;
            Dev::HistLeafStep step{{o.begin, o.end, (uint32_t)ws, o.pick.edge, nl}, o.slot, Dev::HIST_NO_SLOT, el, er};
            step.bounds[0] = step.bounds[1] = o.bd;
            step.parent_out = o.out;
            if (mono_on_) child_bounds(o, n, mono_[ws], o.pick, &step.bounds[0], &step.bounds[1]);
            if (el || er) {
                if (free_slots.empty()) fail_str("LambdaMART histogram grower: internal error: the histogram pool is exhausted");
                step.small_slot = free_slots.back();
                free_slots.pop_back();
            }
            if (!dev_.hist_leaf_step(step, how_, pick, &err)) fail_str(err);
            const uint32_t slot_l = left_small ? step.small_slot : o.slot, slot_r = left_small ? o.slot : step.small_slot;
            if (el) consider({o.node->lhs.get(), slot_l, o.begin, mid, o.depth + 1, step.bounds[0], il, 0.0, pick[0], o.out, true});
            else lv->close(o.node->lhs.get(), o.begin, mid, step.bounds[0], o.out, true);
            if (er) consider({o.node->rhs.get(), slot_r, mid, o.end, o.depth + 1, step.bounds[1], ir, 0.0, pick[1], o.out, true});
            else lv->close(o.node->rhs.get(), mid, o.end, step.bounds[1], o.out, true);
            // a slot whose child was not searched holds nothing that is read again
            if (!el && (el || er)) free_slots.push_back(slot_l);
            if (!er && (el || er)) free_slots.push_back(slot_r);
            if (!el && !er) free_slots.push_back(o.slot);
        }
        for (const Open& o : open) lv->close(o);
        pool_bytes_ = std::max(pool_bytes_, (uint64_t)slots * features() * k_ * (newton_.on ? 20u : 12u));
        return true;
    }

    // The tree's features: their number, and slot fi of them as a slot of the bins.
    size_t features() const { return sel_.empty() ? feats_.size() : sel_.size(); }
    size_t full(size_t fi) const { return sel_.empty() ? fi : (size_t)sel_[fi]; }

    // Leaf t, holding n instances, becomes an inner node with two fresh leaves: feature fi of the tree's, bins 0..edge of it
    // go left, nl instances.  Returns the feature's slot in the bin matrix.
    size_t split_node(TreeNode* t, size_t fi, uint32_t edge, uint32_t n, uint32_t nl) {
        if (fi >= features() || edge >= nedges_[full(fi)] || nl == 0 || nl >= n)
            fail_str("LambdaMART histogram grower: internal error: an impossible split");
        const size_t ws = full(fi);
        t->leaf = false;
        t->fid = feats_[ws];
        t->value = (double)edges_[ws * 256 + edge];
        t->lhs.reset(new TreeNode());
        t->rhs.reset(new TreeNode());
        return ws;
    }

    // The selection rule's second half, one place for the level loop and the leaf-wise one: *gain = what record b gains over
    // its own node (n instances, interval bd); returns whether the node may split on it.  Newton gain: imp less the node's
    // own term (Qnode, Wnode; under monotone constraints the clamped one), which must exceed min_split_gain.  Variance:
    // imp less Qnode^2 / n, for ranking the open leaves only (rounding may leave it slightly below 0): any valid record splits.
    // Leaf regularisation: the node's own term is the one at its carried output, which is left in o->out.
    bool may_split(const Dev::HistCand& b, uint32_t n, Open* o, double* gain) const {
        if (!b.valid) return false;
        if (newton_.on && reg_on_) {
            o->out = node_output(b, n, *o);
            *gain = b.imp - reg_own_term(b.qtot, b.wtot, how_.s_l, how_.s_w, newton_.lambda_l2, reg_, o->out);
            return *gain > newton_.min_split_gain;
        }
        if (newton_.on) {
            *gain = b.imp - (mono_on_ ? monotone_term(b.qtot, b.wtot, o->bd) : newton_term(b.qtot, b.wtot));
            return *gain > newton_.min_split_gain;
        }
        const double sn = (double)b.qtot;
        *gain = b.imp - (sn * sn) / (double)n;
        return true;
    }

    // (G G) / (H + lambda_l2) of an integer pair, every operation rounded on its own
    double newton_term(long long q, long long w) const {
        const double g = std::ldexp((double)q, -how_.s_l);
        return (g * g) / (std::ldexp((double)w, -how_.s_w) + newton_.lambda_l2);
    }

    // Monotone constraints.  The root's interval; a value clamped to an interval; and term(G, H, v) of an output
    // G / (H + lambda_l2) (the leaf rule's 0.0 for a zero denominator) clamped to v: the Newton term when nothing was clamped,
    // else (2 G) v - ((H + lambda_l2) v) v, every operation rounded on its own, as the monotone scan kernels do.
    static Dev::HistBounds whole_line() { return {-std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity()}; }
    static double clamp(double out, const Dev::HistBounds& bd) {
        const double v = out < bd.lo ? bd.lo : out;
        return v > bd.hi ? bd.hi : v;
    }
    double monotone_term(long long q, long long w, const Dev::HistBounds& bd, double* v_out = nullptr) const {
        const double g = std::ldexp((double)q, -how_.s_l), den = std::ldexp((double)w, -how_.s_w) + newton_.lambda_l2;
        const double out = den != 0.0 ? g / den : 0.0, v = clamp(out, bd);
        if (v_out) *v_out = v;
        return v == out ? (g * g) / den : (2.0 * g) * v - (den * v) * v;
    }
    // Leaf regularisation.  The output node o (n instances, totals in record b) carries: its own v, the parent's pull included
    // (for the root, which has no parent, without it).  The children inherit it as their parent's output.
    double node_output(const Dev::HistCand& b, uint32_t n, const Open& o) const {
        return reg_side(b.qtot, b.wtot, n, how_.s_l, how_.s_w, newton_.lambda_l2, reg_, o.has_parent ? &o.parent_out : nullptr, o.bd.lo, o.bd.hi).v;
    }
    // the children's intervals after the split b of node o (n instances) on a feature of sign c: mid = (vL + vR) 0.5 cuts the
    // node's interval
    void child_bounds(const Open& o, uint32_t n, int c, const Dev::HistCand& b, Dev::HistBounds* lhs, Dev::HistBounds* rhs) const {
        const Dev::HistBounds& bd = o.bd;
        *lhs = *rhs = bd;
        if (c == 0) return;
        double vl = 0.0, vr = 0.0;
        if (reg_on_) {  // (both sides are pulled toward the splitting node's carried output)
            vl = reg_side(b.ql, b.wl, b.nl, how_.s_l, how_.s_w, newton_.lambda_l2, reg_, &o.out, bd.lo, bd.hi).v;
            vr = reg_side(b.qtot - b.ql, b.wtot - b.wl, n - b.nl, how_.s_l, how_.s_w, newton_.lambda_l2, reg_, &o.out, bd.lo, bd.hi).v;
        } else {
            (void)monotone_term(b.ql, b.wl, bd, &vl);
            (void)monotone_term(b.qtot - b.ql, b.wtot - b.wl, bd, &vr);
        }
        const double mid = (vl + vr) * 0.5;
        if (c > 0) lhs->hi = mid, rhs->lo = mid;
        else lhs->lo = mid, rhs->hi = mid;
    }

    // Leaf values from the leaves' integer sums of Q and W, under the leaves' exponents (the search's own unless the gradients
    // are quantised).  rooted = false: the tree never searched, and the index list the sums are
    // taken over is made here, as the root's.
    // Under monotone constraints a value is clamped to its leaf's interval, and the moved ones are counted.
    void leaf_values(const Leaves& lv, bool rooted, HistTreeReport* rep) {
        std::string err;
        auto t0 = std::chrono::steady_clock::now();
        if (!rooted && !dev_.hist_root(false, &err)) fail_str(err);
        std::vector<long long> qw;
        if (!dev_.hist_leaf_sums(lv.stretches, &qw, &err)) fail_str(err);
        for (size_t i = 0; i < lv.nodes.size(); i++) {
            const long long q = qw[i * 2], w = qw[i * 2 + 1];
            if (newton_.on && reg_on_) {
                const uint32_t n = lv.stretches[i].end - lv.stretches[i].begin;
                const double* parent = lv.has_parent[i] ? &lv.parent_out[i] : nullptr;
                const Dev::HistBounds line = whole_line();
                const double v = reg_side(q, w, n, leaf_s_l_, leaf_s_w_, newton_.lambda_l2, reg_, parent, lv.bounds[i].lo, lv.bounds[i].hi).v;
                if (mono_on_ && v != reg_side(q, w, n, leaf_s_l_, leaf_s_w_, newton_.lambda_l2, reg_, parent, line.lo, line.hi).v) rep->clamped_leaves++;
                lv.nodes[i]->value = v;
            } else if (newton_.on) {
                const double den = std::ldexp((double)w, -leaf_s_w_) + newton_.lambda_l2;
                const double out = den != 0.0 ? std::ldexp((double)q, -leaf_s_l_) / den : 0.0;
                const double v = mono_on_ ? clamp(out, lv.bounds[i]) : out;
                if (mono_on_ && v != out) rep->clamped_leaves++;
                lv.nodes[i]->value = v;
            } else {
                lv.nodes[i]->value = w != 0 ? std::ldexp((double)q, -leaf_s_l_) / std::ldexp((double)w, -leaf_s_w_) : 0.0;
            }
        }
        rep->leaf_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }

    void check_features(const std::vector<uint32_t>* features) const {
        for (uint32_t s : sel_)
            if (s >= feats_.size()) fail_str("LambdaMART histogram grower: a sampled feature outside the feature list");
        if (features && sel_.empty()) fail_str("LambdaMART histogram grower: an empty feature sample");
    }
    // rf_train.hpp's rule: may a node be searched at all?
    bool enterable(uint32_t n, uint32_t depth) const { return n >= 2 && depth < max_depth_ && n >= min_leaf_; }

    Dev& dev_;
    std::vector<uint32_t> feats_;
    uint32_t k_, max_depth_, min_leaf_, n_ = 0, n_full_ = 0;  // n_: the tree's instances (n_full_ of them without a query sample)
    uint32_t n_sample_ = 0;                                    // the sample's instances: n_ unless the tree is a GOSS one
    HistNewton newton_;
    Dev::HistSearch how_{};                                    // the tree's search parameters, its exponents s_l / s_w among them
    int leaf_s_l_ = 0, leaf_s_w_ = 0;                          // the exponents of the leaf sums (quantised gradients: not the search's)
    uint32_t max_leaves_ = 0;                                  // 0: level-wise growth
    uint64_t pool_bytes_ = 0;
    bool mono_on_ = false;                                     // some monotone sign is not 0
    std::vector<int> mono_;                                    // (then) the signs, by entry of feats_
    bool symmetric_ = false;                                   // every node of a level splits on one candidate
    HistReg reg_;                                              // leaf regularisation's three numbers
    bool reg_on_ = false;                                      // one of them is not 0
    uint32_t quant_bits_ = 0;                                  // quantised gradients: bits per value (0: off)
    std::vector<uint32_t> sel_;                                // the tree's features as slots of the bins (empty: all)
    std::vector<float> edges_;
    std::vector<uint32_t> nedges_;
};

}  // namespace fr
