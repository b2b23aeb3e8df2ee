// A program of its own over csrc/permute_host.hpp (the options, the refusals, the stream, the positions and the report of
// DESIGN.md section 16), for -fsanitize=address,undefined: no documents and one, equal keys forced through the tie rule, the
// report at one repeat, every refusal.  tests/test_permute_host.py builds and runs it.
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "permute_host.hpp"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static bool options_refused(const char* text, const char* needle) {
    try {
        fr::permute_options_from_json(frjson::parse(text));
    } catch (const fr::FrError& e) {
        return e.debug.find(needle) != std::string::npos;
    } catch (const frjson::ParseError&) {
        return std::strcmp(needle, "parse") == 0;
    }
    return false;
}

static bool features_refused(const char* text, const std::vector<uint32_t>& have, const char* needle) {
    try {
        fr::permute_features(fr::permute_options_from_json(frjson::parse(text)), have);
    } catch (const fr::FrError& e) {
        return e.debug.find(needle) != std::string::npos;
    }
    return false;
}

static bool shape_refused(const fr::Model& m, const char* needle) {
    try {
        fr::permute_model_shape(m);
    } catch (const fr::FrError& e) {
        return e.debug.find(needle) != std::string::npos;
    }
    return false;
}

static std::shared_ptr<fr::TreeNode> stump(uint32_t fid) {
    auto n = std::make_shared<fr::TreeNode>();
    n->leaf = false, n->fid = fid, n->value = 0.5;
    n->lhs = std::make_unique<fr::TreeNode>();
    n->rhs = std::make_unique<fr::TreeNode>();
    n->rhs->value = 1.0;
    return n;
}

int main() {
    // the stream key: splitmix64's third output for seed 0 is mix(3 G); it is neither of the resampling keys
    CHECK(frpermute::stream_key(0) == frresample::mix(3ull * frresample::GOLDEN));
    CHECK(frpermute::stream_key(0) != frresample::boot_key(0) && frpermute::stream_key(0) != frresample::perm_key(0));
    CHECK(frpermute::stream_key(~0ull) == frresample::mix(3ull * frresample::GOLDEN - 1ull));  // mod 2^64

    // no documents, one document
    fr::permute_sources(0, 0, nullptr, 0, nullptr);
    fr::permute_sources_from_keys(nullptr, nullptr, 0, nullptr);
    uint32_t one = 7;
    const uint32_t q0 = 3;
    fr::permute_sources(5, 2, nullptr, 1, &one);
    CHECK(one == 0);
    one = 7;
    fr::permute_sources(5, 2, &q0, 1, &one);
    CHECK(one == 0);

    // equal keys: the index decides
    {
        const uint64_t keys[6] = {9, 4, 9, 4, 4, 1};
        uint32_t src[6];
        fr::permute_sources_from_keys(keys, nullptr, 6, src);
        const uint32_t want[6] = {5, 1, 3, 4, 0, 2};
        CHECK(std::memcmp(src, want, sizeof want) == 0);
        // two interleaved queries: members {0, 2, 4} have keys {9, 9, 4} -> sorted (4,4) (9,0) (9,2); {1, 3, 5}: {4, 4, 1} -> 5 1 3
        const uint32_t query_of[6] = {8, 2, 8, 2, 8, 2};
        fr::permute_sources_from_keys(keys, query_of, 6, src);
        const uint32_t want_q[6] = {4, 5, 0, 1, 2, 3};
        CHECK(std::memcmp(src, want_q, sizeof want_q) == 0);
        std::vector<std::pair<uint64_t, uint32_t>> kv = {{2, 1}, {2, 0}, {1, 5}};
        fr::permute_sort(kv);
        CHECK(kv[0].second == 5 && kv[1].second == 0 && kv[2].second == 1);
    }

    // a real stream is a permutation, and stays inside the queries under scope "query"
    {
        const size_t n = 257;
        std::vector<uint32_t> src(n), query_of(n), seen(n, 0);
        for (size_t i = 0; i < n; i++) query_of[i] = (uint32_t)(i % 5);
        fr::permute_sources(11, 63, nullptr, n, src.data());
        for (uint32_t s : src) seen[s]++;
        for (uint32_t c : seen) CHECK(c == 1);
        fr::permute_sources(11, 63, query_of.data(), n, src.data());
        std::fill(seen.begin(), seen.end(), 0);
        for (size_t i = 0; i < n; i++) {
            CHECK(query_of[src[i]] == query_of[i]);
            seen[src[i]]++;
        }
        for (uint32_t c : seen) CHECK(c == 1);
    }

    // positions: ids {2, 5, 9} at positions {4, 1, 6} of 8; src index {2, 0, 1}: 2 <- 9, 5 <- 2, 9 <- 5
    {
        const uint32_t N = 0xFFFFFFFFu;
        const uint32_t at[8] = {N, 5, N, N, 2, N, 9, N}, ids[3] = {2, 5, 9}, src_index[3] = {2, 0, 1};
        uint32_t out[8];
        const std::vector<uint32_t> pos = fr::permute_position_table(at, 8, ids, 3);
        CHECK(pos.size() == 3 && pos[0] == 4 && pos[1] == 1 && pos[2] == 6);
        fr::permute_positions(pos.data(), src_index, 3, 8, out);
        const uint32_t want[8] = {0, 4, 2, 3, 6, 5, 1, 7};
        CHECK(std::memcmp(out, want, sizeof want) == 0);
        bool refused = false;
        try {
            const uint32_t other[3] = {2, 5, 8};
            fr::permute_position_table(at, 8, other, 3);
        } catch (const fr::FrError& e) {
            refused = e.debug.find("instance 8 has no position") != std::string::npos;
        }
        CHECK(refused);
        refused = false;
        try {
            fr::permute_position_table(at, 8, ids, 2);
        } catch (const fr::FrError& e) {
            refused = e.debug.find("holds 3 documents, the view 2") != std::string::npos;
        }
        CHECK(refused);
        CHECK(fr::permute_position_table(nullptr, 0, nullptr, 0).empty());
        fr::permute_positions(nullptr, nullptr, 0, 0, nullptr);
    }

    // the report: one repeat has no deviation; three repeats by hand
    {
        const double v1[1] = {0.25};
        fr::PermuteScore s = fr::permute_report(0.75, v1, 1);
        CHECK(s.importance == 0.5 && s.std == 0.0);
        const double v3[3] = {0.5, 0.25, 0.75};  // d = 0.25, 0.5, 0: mean 0.25; squares 0, 0.0625, 0.0625: sqrt(0.125 / 2) = 0.25
        s = fr::permute_report(0.75, v3, 3);
        CHECK(s.importance == 0.25 && s.std == 0.25);
        const double vb[2] = {0.75, 0.75};
        s = fr::permute_report(0.75, vb, 2);
        CHECK(s.importance == 0.0 && s.std == 0.0);
    }

    // options: defaults, every key, every refusal
    {
        fr::PermuteOptions o = fr::permute_options_from_json(frjson::parse("{}"));
        CHECK(o.repeats == 5 && o.seed == 0 && !o.per_query && !o.has_features && o.skip_unused && o.max_slots == 0);
        o = fr::permute_options_from_json(frjson::parse(
            "{\"repeats\": 64, \"seed\": 18446744073709551615, \"scope\": \"query\", \"features\": [3, 1], \"skip_unused\": false, \"max_slots\": 3}"));
        CHECK(o.repeats == 64 && o.seed == ~0ull && o.per_query && o.has_features && o.features.size() == 2 && !o.skip_unused && o.max_slots == 3);
        CHECK(options_refused("{\"repeats\": 0}", "repeats must be between 1 and 64, not 0"));
        CHECK(options_refused("{\"repeats\": 65}", "repeats must be between 1 and 64, not 65"));
        CHECK(options_refused("{\"repeats\": -1}", "expected unsigned integer for repeats"));
        CHECK(options_refused("{\"scope\": \"list\"}", "scope must be \\\"dataset\\\" or \\\"query\\\", not \\\"list\\\"") ||
              options_refused("{\"scope\": \"list\"}", "scope must be \"dataset\" or \"query\", not \"list\""));
        CHECK(options_refused("{\"scope\": 1}", "expected a string for scope"));
        CHECK(options_refused("{\"features\": 3}", "expected a sequence for features"));
        CHECK(options_refused("{\"features\": [4294967296]}", "expected u32"));
        CHECK(options_refused("{\"skip_unused\": 1}", "expected a boolean for skip_unused"));
        CHECK(options_refused("{\"max_slots\": 0}", "max_slots must be at least 1"));
        CHECK(options_refused("{\"repeat\": 2}", "unknown field `repeat`"));
        CHECK(options_refused("[]", "expected a map for the permutation options"));
        CHECK(options_refused("{", "parse"));
        const std::vector<uint32_t> have = {4, 0, 2};
        std::vector<uint32_t> f = fr::permute_features(fr::permute_options_from_json(frjson::parse("{}")), have);
        CHECK(f.size() == 3 && f[0] == 0 && f[1] == 2 && f[2] == 4);
        f = fr::permute_features(fr::permute_options_from_json(frjson::parse("{\"features\": [4, 0]}")), have);
        CHECK(f.size() == 2 && f[0] == 4 && f[1] == 0);
        f = fr::permute_features(fr::permute_options_from_json(frjson::parse("{\"features\": []}")), have);
        CHECK(f.empty());
        CHECK(features_refused("{\"features\": [1]}", have, "feature 1 is not one of the dataset's features"));
        CHECK(features_refused("{\"features\": [2, 4, 2]}", have, "feature 2 is listed twice"));
    }

    // model shapes, and which features a model reads
    {
        fr::Model lin, single, tree, forest, mixed, nested, flat, empty;
        lin.kind = fr::Model::Linear, lin.weights = {0.5, 0.0, -0.0, 2.0};
        single.kind = fr::Model::SingleFeature, single.fid = 2, single.dir = -1.0;
        tree.kind = fr::Model::DecisionTree, tree.tree = stump(1);
        forest.kind = fr::Model::Ensemble, forest.members = {tree, tree}, forest.ens_weights = {1.0, 2.0};
        forest.members[1].tree = stump(3);
        mixed.kind = fr::Model::Ensemble, mixed.members = {lin, tree}, mixed.ens_weights = {1.0, 1.0};
        nested.kind = fr::Model::Ensemble, nested.members = {forest}, nested.ens_weights = {1.0};
        flat.kind = fr::Model::Ensemble, flat.members = {lin, single}, flat.ens_weights = {1.0, 1.0};
        empty.kind = fr::Model::Ensemble;
        CHECK(fr::permute_model_shape(lin) == fr::PermuteShape::LINEAR && fr::permute_model_shape(single) == fr::PermuteShape::SINGLE);
        CHECK(fr::permute_model_shape(tree) == fr::PermuteShape::TREES && fr::permute_model_shape(forest) == fr::PermuteShape::TREES);
        CHECK(fr::permute_model_shape(flat) == fr::PermuteShape::ENSEMBLE_LINEAR);
        CHECK(shape_refused(mixed, "not Ensemble[Linear, DecisionTree]"));
        CHECK(shape_refused(nested, "not Ensemble[Ensemble[DecisionTree, DecisionTree]]"));
        CHECK(shape_refused(empty, "not Ensemble[]"));
        const double inf = std::numeric_limits<double>::infinity();
        const std::vector<double> colmax = {1.0, inf, 3.0, 4.0};
        CHECK(fr::permute_feature_used(lin, 0, colmax) && fr::permute_feature_used(lin, 3, colmax));
        CHECK(fr::permute_feature_used(lin, 1, colmax));   // a zero weight on a column that holds inf or NaN: 0 * inf is NaN
        CHECK(!fr::permute_feature_used(lin, 2, colmax));  // -0.0 is zero
        CHECK(!fr::permute_feature_used(lin, 4, colmax));  // past the matrix
        lin.weights.resize(2);
        CHECK(!fr::permute_feature_used(lin, 3, colmax));  // past the weights: weight 0
        CHECK(fr::permute_feature_used(single, 2, colmax) && !fr::permute_feature_used(single, 0, colmax));
        CHECK(fr::permute_feature_used(tree, 1, colmax) && !fr::permute_feature_used(tree, 3, colmax));
        CHECK(fr::permute_feature_used(forest, 3, colmax) && !fr::permute_feature_used(forest, 0, colmax));
        forest.ens_weights.resize(1);  // zip stops at the shorter: the second tree is not part of the model
        CHECK(!fr::permute_feature_used(forest, 3, colmax));
        CHECK(fr::permute_feature_used(flat, 2, colmax));
    }

    // the model as the kernels take it, at its edges
    {
        using PM = frdev::PermuteMember;
        fr::Model lin, single, tree, forest, flat;
        lin.kind = fr::Model::Linear, lin.weights = {0.5, -1.0};
        single.kind = fr::Model::SingleFeature, single.fid = 2, single.dir = -1.0;
        tree.kind = fr::Model::DecisionTree, tree.tree = stump(1);
        // a bare tree: one TREES member over one root, taken raw
        fr::PermuteModel pm = fr::permute_model(tree, fr::permute_model_shape(tree), 4);
        CHECK(pm.members.size() == 1 && pm.members[0].kind == PM::TREES && pm.members[0].trees == pm.trees.get() && pm.weights.empty());
        CHECK(pm.trees->raw_single && pm.trees->root.size() == 1 && pm.trees->root[0] == 0 && pm.trees->fid.size() == 3 && pm.trees->fid[0] == 1);
        // a forest with fewer weights than members, and the reverse: zip stops at the shorter
        forest.kind = fr::Model::Ensemble, forest.members = {tree, tree, tree}, forest.ens_weights = {2.0, 3.0};
        forest.members[1].tree = stump(3);
        pm = fr::permute_model(forest, fr::permute_model_shape(forest), 4);
        CHECK(pm.members.size() == 1 && pm.members[0].kind == PM::TREES && pm.members[0].trees == pm.trees.get() && !pm.trees->raw_single);
        CHECK(pm.trees->root.size() == 2 && pm.trees->weight.size() == 2 && pm.trees->weight[0] == 2.0 && pm.trees->weight[1] == 3.0);
        CHECK(pm.trees->fid[(size_t)pm.trees->root[0]] == 1 && pm.trees->fid[(size_t)pm.trees->root[1]] == 3);
        forest.members.resize(1), forest.ens_weights = {2.0, 3.0, 4.0};
        pm = fr::permute_model(forest, fr::permute_model_shape(forest), 4);
        CHECK(pm.trees->root.size() == 1 && pm.trees->weight.size() == 1 && pm.trees->weight[0] == 2.0);
        // a linear model with fewer weights than d (the rest are 0.0) and with more (the rest are dropped)
        pm = fr::permute_model(lin, fr::permute_model_shape(lin), 4);
        CHECK(pm.members.size() == 1 && pm.members[0].kind == PM::LINEAR && pm.members[0].ens_weight == 1.0 && !pm.trees);
        CHECK(pm.weights.size() == 1 && pm.weights[0].size() == 4 && pm.members[0].weights == pm.weights[0].data());
        CHECK(pm.weights[0][0] == 0.5 && pm.weights[0][1] == -1.0 && pm.weights[0][2] == 0.0 && pm.weights[0][3] == 0.0);
        pm = fr::permute_model(lin, fr::permute_model_shape(lin), 1);
        CHECK(pm.weights[0].size() == 1 && pm.weights[0][0] == 0.5 && pm.members[0].weights == pm.weights[0].data());
        pm = fr::permute_model(lin, fr::permute_model_shape(lin), 0);
        CHECK(pm.members.size() == 1 && pm.weights[0].empty());
        pm = fr::permute_model(single, fr::permute_model_shape(single), 4);
        CHECK(pm.members.size() == 1 && pm.members[0].kind == PM::SINGLE && pm.members[0].fid == 2 && pm.members[0].dir == -1.0 && pm.weights.empty());
        // a mixed ensemble, more members than weights: each LINEAR member points at its own weights, in member order, after
        // the store has grown (many members) and after the record has moved
        flat.kind = fr::Model::Ensemble;
        for (int k = 0; k < 40; k++) {
            flat.members.push_back(k % 3 == 1 ? single : lin);
            flat.members.back().weights.assign(lin.weights.size(), (double)k);
            flat.ens_weights.push_back(0.25 * k);
        }
        flat.ens_weights.resize(37);
        fr::PermuteModel moved = fr::permute_model(flat, fr::permute_model_shape(flat), 3);
        pm = std::move(moved);
        CHECK(pm.members.size() == 37 && pm.weights.size() == 25 && !pm.trees);
        size_t at = 0;
        for (size_t k = 0; k < pm.members.size(); k++) {
            CHECK(pm.members[k].ens_weight == 0.25 * (double)k);
            if (k % 3 == 1) {
                CHECK(pm.members[k].kind == PM::SINGLE && pm.members[k].weights == nullptr && pm.members[k].fid == 2);
                continue;
            }
            CHECK(pm.members[k].kind == PM::LINEAR && pm.members[k].weights == pm.weights[at].data() && pm.weights[at].size() == 3);
            CHECK(pm.members[k].weights[0] == (double)k && pm.members[k].weights[1] == (double)k && pm.members[k].weights[2] == 0.0);
            at++;
        }
        CHECK(at == pm.weights.size());
    }
    std::printf("permute_host ok\n");
    return 0;
}
