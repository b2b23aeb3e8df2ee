// Models (src/model.rs:10-112) and their serde wire form, the error every call carries to the C
// boundary, and the field helpers every wire form is read with.  Plain C++ over json.hpp: host.hpp and ca_restart.hpp
// both include it.
#pragma once
#include <cmath>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "json.hpp"

namespace fr {

using frjson::Value;

// Error carried to the C boundary; `debug` is already in Rust `{:?}` form (src/ffi.rs:45-74).
struct FrError {
    std::string debug;
};
[[noreturn]] inline void fail_str(const std::string& msg) { throw FrError{frjson::rust_debug_str(msg)}; }
[[noreturn]] inline void fail_raw(const std::string& debug) { throw FrError{debug}; }

struct TreeNode {
    bool leaf = true;
    double value = 0.0;  // leaf value or split threshold
    uint32_t fid = 0;
    std::unique_ptr<TreeNode> lhs, rhs;
};

struct Model {
    enum Kind { SingleFeature, Linear, DecisionTree, Ensemble, NeuralNet } kind = Linear;
    uint32_t fid = 0;
    double dir = 0.0;
    std::vector<double> weights;
    std::shared_ptr<TreeNode> tree;
    std::vector<double> ens_weights;
    std::vector<Model> members;
    // NeuralNet: s = b2 + sum_j relu(b1_j + sum_i x_i W1_ji) w2_j.  nn_w1: nn_b1.size() rows of nn_cols
    // numbers, row j = hidden unit j, column i = feature id i.
    size_t nn_cols = 0;
    std::vector<double> nn_w1, nn_b1, nn_w2;
    double nn_b2 = 0.0;
    // ... with a second hidden layer (nn_hb2 not empty): s = b2 + sum_k fl(relu(c_k + sum_j relu(z_j) W2_kj) w2_k).  nn_hw2: W2,
    // nn_hb2.size() rows of nn_b1.size() numbers, row k = unit k of the second layer; nn_hb2: c; nn_w2 then holds one number per
    // unit of the second layer.
    std::vector<double> nn_hw2, nn_hb2;
    size_t nn_hidden2() const { return nn_hb2.size(); }
};

inline double json_f64(const Value& v, const char* what) {
    if (!v.is_number()) fail_raw(std::string("Error(\"invalid type: expected f64 for ") + what + "\", line: 0, column: 0)");
    return v.as_double();
}
inline uint64_t json_u64(const Value& v, const char* what) {
    if (v.kind == Value::UInt) return v.u;
    if (v.kind == Value::Int && v.i >= 0) return (uint64_t)v.i;
    fail_raw(std::string("Error(\"invalid type: expected unsigned integer for ") + what + "\", line: 0, column: 0)");
}
// serde rejects integers that do not fit the field's type instead of truncating them
inline uint32_t json_u32(const Value& v, const char* what) {
    const uint64_t x = json_u64(v, what);
    if (x > (uint64_t)UINT32_MAX)
        fail_raw("Error(\"invalid value: integer `" + std::to_string(x) + "`, expected u32\", line: 0, column: 0)");
    return (uint32_t)x;
}
inline bool json_bool(const Value& v, const char* what) {
    if (v.kind != Value::Bool) fail_raw(std::string("Error(\"invalid type: expected a boolean for ") + what + "\", line: 0, column: 0)");
    return v.b;
}
inline const Value& json_field(const Value& obj, const char* key) {
    const Value* f = obj.find(key);
    if (!f) fail_raw(std::string("Error(\"missing field `") + key + "`\", line: 0, column: 0)");
    return *f;
}
// serde externally-tagged enum: {"Variant": payload}
inline const frjson::Member& json_variant(const Value& v, const char* what) {
    if (!v.is_object() || v.obj.size() != 1)
        fail_raw(std::string("Error(\"expected a single-key map for enum ") + what + "\", line: 0, column: 0)");
    return v.obj[0];
}

inline std::unique_ptr<TreeNode> tree_from_json(const Value& v) {
    const auto& var = json_variant(v, "TreeNode");
    auto node = std::make_unique<TreeNode>();
    if (var.first == "LeafNode") {
        node->leaf = true;
        node->value = json_f64(var.second, "LeafNode");
    } else if (var.first == "FeatureSplit") {
        node->leaf = false;
        node->fid = json_u32(json_field(var.second, "fid"), "fid");
        node->value = json_f64(json_field(var.second, "split"), "split");
        node->lhs = tree_from_json(json_field(var.second, "lhs"));
        node->rhs = tree_from_json(json_field(var.second, "rhs"));
    } else {
        fail_raw("Error(\"unknown variant `" + var.first + "`, expected `FeatureSplit` or `LeafNode`\", line: 0, column: 0)");
    }
    return node;
}

inline Value tree_to_json(const TreeNode& n) {
    Value v = Value::object();
    if (n.leaf) {
        v.set("LeafNode", Value::number(n.value));
    } else {
        Value fs = Value::object();
        fs.set("fid", Value::uint(n.fid));
        fs.set("split", Value::number(n.value));
        fs.set("lhs", tree_to_json(*n.lhs));
        fs.set("rhs", tree_to_json(*n.rhs));
        v.set("FeatureSplit", std::move(fs));
    }
    return v;
}

inline Model model_from_json(const Value& v) {
    const auto& var = json_variant(v, "ModelEnum");
    Model m;
    if (var.first == "Linear") {
        m.kind = Model::Linear;
        const Value& w = json_field(var.second, "weights");
        if (!w.is_array()) fail_raw("Error(\"invalid type: expected a sequence for weights\", line: 0, column: 0)");
        for (const auto& x : w.arr) m.weights.push_back(json_f64(x, "weights"));
    } else if (var.first == "SingleFeature") {
        m.kind = Model::SingleFeature;
        m.fid = json_u32(json_field(var.second, "fid"), "fid");
        m.dir = json_f64(json_field(var.second, "dir"), "dir");
    } else if (var.first == "DecisionTree") {
        m.kind = Model::DecisionTree;
        m.tree = std::shared_ptr<TreeNode>(tree_from_json(var.second).release());
    } else if (var.first == "Ensemble") {
        m.kind = Model::Ensemble;
        const Value& w = json_field(var.second, "weights");
        const Value& ms = json_field(var.second, "models");
        if (!w.is_array() || !ms.is_array())
            fail_raw("Error(\"invalid type: expected sequences in Ensemble\", line: 0, column: 0)");
        for (const auto& x : w.arr) m.ens_weights.push_back(json_f64(x, "weights"));
        for (const auto& x : ms.arr) m.members.push_back(model_from_json(x));
    } else if (var.first == "NeuralNet") {
        m.kind = Model::NeuralNet;
        const Value& act = json_field(var.second, "activation");
        if (!act.is_string() || act.s != "relu") fail_str("NeuralNet: the activation must be \"relu\"");
        const Value& w1 = json_field(var.second, "hidden_weights");
        const Value& b1 = json_field(var.second, "hidden_bias");
        const Value& w2 = json_field(var.second, "output_weights");
        if (!w1.is_array() || !b1.is_array() || !w2.is_array()) fail_raw("Error(\"invalid type: expected sequences in NeuralNet\", line: 0, column: 0)");
        if (w1.arr.empty()) fail_str("NeuralNet: at least one hidden unit is needed");
        const Value *hw2 = var.second.find("hidden2_weights"), *hb2 = var.second.find("hidden2_bias");
        if ((hw2 == nullptr) != (hb2 == nullptr)) fail_str("NeuralNet: hidden2_weights and hidden2_bias must appear together");
        if (hw2 == nullptr) {
            if (b1.arr.size() != w1.arr.size() || w2.arr.size() != w1.arr.size())
                fail_str("NeuralNet: hidden_bias and output_weights must hold one number per row of hidden_weights");
        } else {
            if (!hw2->is_array() || !hb2->is_array()) fail_raw("Error(\"invalid type: expected sequences in NeuralNet\", line: 0, column: 0)");
            if (hw2->arr.size() < 1 || hw2->arr.size() > 64) fail_str("NeuralNet: hidden2_weights must have between 1 and 64 rows");
            if (b1.arr.size() != w1.arr.size()) fail_str("NeuralNet: hidden_bias must hold one number per row of hidden_weights");
            if (hb2->arr.size() != hw2->arr.size() || w2.arr.size() != hw2->arr.size())
                fail_str("NeuralNet: hidden2_bias and output_weights must hold one number per row of hidden2_weights");
        }
        auto finite = [](double x) {
            if (!std::isfinite(x)) fail_str("NeuralNet: every number must be finite");
            return x;
        };
        for (const auto& row : w1.arr) {
            if (!row.is_array()) fail_raw("Error(\"invalid type: expected a sequence for hidden_weights\", line: 0, column: 0)");
            if (&row == &w1.arr[0]) m.nn_cols = row.arr.size();
            if (row.arr.size() != m.nn_cols) fail_str("NeuralNet: the rows of hidden_weights must have one length");
            for (const auto& x : row.arr) m.nn_w1.push_back(finite(json_f64(x, "hidden_weights")));
        }
        for (const auto& x : b1.arr) m.nn_b1.push_back(finite(json_f64(x, "hidden_bias")));
        if (hw2 != nullptr) {
            for (const auto& row : hw2->arr) {
                if (!row.is_array()) fail_raw("Error(\"invalid type: expected a sequence for hidden2_weights\", line: 0, column: 0)");
                if (row.arr.size() != m.nn_b1.size()) fail_str("NeuralNet: every row of hidden2_weights must hold one number per row of hidden_weights");
                for (const auto& x : row.arr) m.nn_hw2.push_back(finite(json_f64(x, "hidden2_weights")));
            }
            for (const auto& x : hb2->arr) m.nn_hb2.push_back(finite(json_f64(x, "hidden2_bias")));
        }
        for (const auto& x : w2.arr) m.nn_w2.push_back(finite(json_f64(x, "output_weights")));
        m.nn_b2 = finite(json_f64(json_field(var.second, "output_bias"), "output_bias"));
    } else {
        fail_raw("Error(\"unknown variant `" + var.first +
                 "`, expected one of `SingleFeature`, `Linear`, `DecisionTree`, `Ensemble`, `NeuralNet`\", line: 0, column: 0)");
    }
    return m;
}

inline Value model_to_json(const Model& m) {
    Value v = Value::object();
    switch (m.kind) {
        case Model::Linear: {
            Value inner = Value::object();
            Value w = Value::array();
            for (double x : m.weights) w.push(Value::number(x));
            inner.set("weights", std::move(w));
            v.set("Linear", std::move(inner));
            break;
        }
        case Model::SingleFeature: {
            Value inner = Value::object();
            inner.set("fid", Value::uint(m.fid));
            inner.set("dir", Value::number(m.dir));
            v.set("SingleFeature", std::move(inner));
            break;
        }
        case Model::DecisionTree:
            v.set("DecisionTree", tree_to_json(*m.tree));
            break;
        case Model::Ensemble: {
            Value inner = Value::object();
            Value w = Value::array();
            for (double x : m.ens_weights) w.push(Value::number(x));
            Value ms = Value::array();
            for (const auto& mm : m.members) ms.push(model_to_json(mm));
            inner.set("weights", std::move(w));
            inner.set("models", std::move(ms));
            v.set("Ensemble", std::move(inner));
            break;
        }
        case Model::NeuralNet: {
            Value inner = Value::object();
            inner.set("activation", Value::string("relu"));
            Value w1 = Value::array(), b1 = Value::array(), w2 = Value::array();
            const size_t h = m.nn_b1.size();
            for (size_t j = 0; j < h; j++) {
                Value row = Value::array();
                for (size_t i = 0; i < m.nn_cols; i++) row.push(Value::number(m.nn_w1[j * m.nn_cols + i]));
                w1.push(std::move(row));
                b1.push(Value::number(m.nn_b1[j]));
            }
            for (double x : m.nn_w2) w2.push(Value::number(x));
            inner.set("hidden_weights", std::move(w1));
            inner.set("hidden_bias", std::move(b1));
            if (m.nn_hidden2() != 0) {
                Value hw2 = Value::array(), hb2 = Value::array();
                for (size_t k = 0; k < m.nn_hidden2(); k++) {
                    Value row = Value::array();
                    for (size_t j = 0; j < h; j++) row.push(Value::number(m.nn_hw2[k * h + j]));
                    hw2.push(std::move(row));
                    hb2.push(Value::number(m.nn_hb2[k]));
                }
                inner.set("hidden2_weights", std::move(hw2));
                inner.set("hidden2_bias", std::move(hb2));
            }
            inner.set("output_weights", std::move(w2));
            inner.set("output_bias", Value::number(m.nn_b2));
            v.set("NeuralNet", std::move(inner));
            break;
        }
    }
    return v;
}

}  // namespace fr
