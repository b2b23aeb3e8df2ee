// A program of its own over csrc/explain_host.hpp (the model check, the cover pass's tree form and the path table of
// DESIGN.md section 12), for -fsanitize=address,undefined: a chain tree at the path limit and one past it, a tree that
// repeats a feature, leaf counts with empty branches.  tests/test_explain_host.py builds and runs it.
#include <cstdio>
#include <memory>

#include "explain_host.hpp"

static std::unique_ptr<fr::TreeNode> leaf(double v) {
    auto n = std::make_unique<fr::TreeNode>();
    n->value = v;
    return n;
}
static std::unique_ptr<fr::TreeNode> split(uint32_t fid, double s, std::unique_ptr<fr::TreeNode> l, std::unique_ptr<fr::TreeNode> r) {
    auto n = std::make_unique<fr::TreeNode>();
    n->leaf = false, n->fid = fid, n->value = s, n->lhs = std::move(l), n->rhs = std::move(r);
    return n;
}
static std::unique_ptr<fr::TreeNode> chain(uint32_t feats) {
    std::unique_ptr<fr::TreeNode> n = leaf(1.0);
    for (uint32_t f = feats; f-- > 0;) n = split(f, 0.0, leaf(-(double)f), std::move(n));
    return n;
}
static fr::Model ensemble(std::vector<std::unique_ptr<fr::TreeNode>> trees) {
    fr::Model m;
    m.kind = fr::Model::Ensemble;
    for (auto& t : trees) {
        fr::Model mm;
        mm.kind = fr::Model::DecisionTree;
        mm.tree = std::shared_ptr<fr::TreeNode>(t.release());
        m.members.push_back(std::move(mm));
        m.ens_weights.push_back(0.5 + (double)m.members.size());
    }
    return m;
}
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main() {
    std::vector<std::unique_ptr<fr::TreeNode>> trees;
    trees.push_back(chain(32));
    trees.push_back(split(0, 0.5, split(0, -0.25, leaf(1.0), split(2, 0.0, leaf(2.0), leaf(-3.0))), split(0, 1.0, split(7, 1.0, leaf(4.0), leaf(0.5)), leaf(7.0))));
    trees.push_back(leaf(3.0));
    const fr::Model m = ensemble(std::move(trees));
    const fr::ExplainModel em = fr::explain_model(m);
    const frdev::ExWalk walk = fr::explain_walk(em);
    CHECK(walk.leaf0.back() == 33 + 6 + 1 && walk.root.size() == 3);
    std::vector<uint32_t> counts(walk.leaf0.back(), 0u);
    for (size_t i = 0; i < counts.size(); i += 3) counts[i] = (uint32_t)(i + 1);  // most branches are empty
    const fr::ExplainPlan plan = fr::explain_plan(em, counts, 5);
    const frdev::ExTables& tab = plan.tab;
    CHECK(tab.max_path == 32 && tab.max_tree_feats == 32 && tab.ncols == 32);
    CHECK(tab.m.size() == 40 && tab.eoff.back() + tab.m.back() == tab.slot.size() && tab.slot.size() == tab.z.size());
    CHECK(tab.feat0.back() == tab.fid.size() && tab.fid[4] == 4 && tab.fid[5] == frdev::EX_NO_FEATURE);
    for (size_t e = 0; e < tab.z.size(); e++) CHECK(tab.z[e] >= 0.0 && tab.z[e] <= 1.0 && tab.lo[e] < tab.hi[e] + 2.0);
    CHECK(plan.bias == plan.bias);
    bool refused = false;
    try {
        std::vector<std::unique_ptr<fr::TreeNode>> deep;
        deep.push_back(chain(33));
        const fr::Model md = ensemble(std::move(deep));
        const fr::ExplainModel emd = fr::explain_model(md);
        fr::explain_plan(emd, std::vector<uint32_t>(34, 1u), 40);
    } catch (const fr::FrError&) {
        refused = true;
    }
    CHECK(refused);
    std::printf("explain_host ok\n");
    return 0;
}
