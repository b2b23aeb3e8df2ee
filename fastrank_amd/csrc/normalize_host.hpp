// Host side of feature normalisation: the finishing of a record (variance, the f32 parameters), the
// chunked statistics of one column as the device takes them, the normaliser and its wire form (the reference's serde shape,
// src/normalizers.rs:7-44, plus {"PerQuery": method}).  No HIP, no environment.
#pragma once
#include <cmath>
#include <map>

#include "host.hpp"
#include "normalize.hpp"

namespace fr {

// src/stats.rs:6-13 ComputedStats
struct ComputedStats {
    uint64_t num_elements = 0;
    double mean = 0.0, variance = 0.0, max = 0.0, min = 0.0, total = 0.0;
};

// src/stats.rs:54-63, :97-102: no record for fewer than two values
inline bool norm_finish(const frdev::NormRecord& r, ComputedStats* out) {
    if (r.n <= 1) return false;
    out->num_elements = r.n, out->mean = r.mean, out->max = r.max, out->min = r.min, out->total = r.total;
    out->variance = r.s / (double)(r.n - 1);
    return true;
}

// One column over a list of m instances, as stats_chunk_kernel and stats_fold_kernel take it: a record per chunk of
// FR_STATS_CHUNK consecutive instances (held[i] == 0: instance i does not hold the feature; held == nullptr: all do),
// folded in chunk order.
inline frdev::NormRecord norm_chunked(const float* vals, const uint8_t* held, size_t m) {
    frdev::NormRecord acc = frdev::norm_empty();
    for (size_t c0 = 0; c0 < m; c0 += frdev::FR_STATS_CHUNK) {
        frdev::NormRecord r = frdev::norm_empty();
        const size_t c1 = std::min<size_t>(m, c0 + frdev::FR_STATS_CHUNK);
        for (size_t i = c0; i < c1; i++)
            if (held == nullptr || held[i]) frdev::norm_push(r, (double)vals[i]);
        frdev::norm_fold(acc, r);
    }
    return acc;
}

struct Normalizer {
    enum Kind { ZScore, MaxMin, Sigmoid, PerQueryZScore, PerQueryMaxMin } kind = ZScore;
    std::map<uint32_t, ComputedStats> stats;  // ZScore / MaxMin

    bool fitted() const { return kind == ZScore || kind == MaxMin; }
    bool per_query() const { return kind == PerQueryZScore || kind == PerQueryMaxMin; }
    const char* method() const {
        switch (kind) {
            case ZScore: case PerQueryZScore: return "zscore";
            case MaxMin: case PerQueryMaxMin: return "maxmin";
            default: return "sigmoid";
        }
    }
};

// src/normalizers.rs:47-54
inline Normalizer::Kind norm_method(const std::string& method) {
    if (method == "zscore") return Normalizer::ZScore;
    if (method == "maxmin" || method == "linear") return Normalizer::MaxMin;
    if (method == "sigmoid") return Normalizer::Sigmoid;
    fail_str("Unsupported Normalizer: " + method);
}

inline Value norm_to_json(const Normalizer& nm) {
    Value o = Value::object();
    if (nm.kind == Normalizer::Sigmoid) {
        o.set("SigmoidNormalizer", Value::array());
        return o;
    }
    if (nm.per_query()) {
        o.set("PerQuery", Value::string(nm.method()));
        return o;
    }
    Value fs = Value::object();
    for (const auto& kv : nm.stats) {
        Value s = Value::object();
        s.set("num_elements", Value::uint(kv.second.num_elements));
        s.set("mean", Value::number(kv.second.mean));
        s.set("variance", Value::number(kv.second.variance));
        s.set("max", Value::number(kv.second.max));
        s.set("min", Value::number(kv.second.min));
        s.set("total", Value::number(kv.second.total));
        fs.set(std::to_string(kv.first), std::move(s));
    }
    Value inner = Value::object();
    inner.set("feature_stats", std::move(fs));
    o.set(nm.kind == Normalizer::ZScore ? "ZScoreNormalizer" : "MaxMinNormalizer", std::move(inner));
    return o;
}

inline double norm_json_stat(const Value& rec, const char* key, const std::string& fid) {
    const Value* v = rec.find(key);
    if (!v || !v->is_number()) fail_str("Normalizer: feature " + fid + " has no finite number for " + key);
    const double x = v->as_double();
    if (!std::isfinite(x)) fail_str("Normalizer: feature " + fid + " has no finite number for " + key);
    return x;
}

inline Normalizer norm_from_json(const Value& v) {
    if (!v.is_object() || v.obj.size() != 1) fail_str("Unsupported Normalizer: expected an object with one variant");
    const std::string& name = v.obj[0].first;
    const Value& body = v.obj[0].second;
    Normalizer nm;
    if (name == "SigmoidNormalizer") {
        if (!body.is_array() || !body.arr.empty()) fail_str("Unsupported Normalizer: SigmoidNormalizer takes []");
        nm.kind = Normalizer::Sigmoid;
        return nm;
    }
    if (name == "PerQuery") {
        if (!body.is_string()) fail_str("Unsupported Normalizer: PerQuery takes a method name");
        const Normalizer::Kind k = norm_method(body.s);
        if (k == Normalizer::Sigmoid) fail_str("Unsupported Normalizer: " + body.s);
        nm.kind = k == Normalizer::ZScore ? Normalizer::PerQueryZScore : Normalizer::PerQueryMaxMin;
        return nm;
    }
    if (name != "ZScoreNormalizer" && name != "MaxMinNormalizer") fail_str("Unsupported Normalizer: " + name);
    nm.kind = name == "ZScoreNormalizer" ? Normalizer::ZScore : Normalizer::MaxMin;
    const Value* fs = body.find("feature_stats");
    if (!fs || !fs->is_object()) fail_str("Normalizer: missing field `feature_stats`");
    for (const auto& kv : fs->obj) {
        uint32_t fid = 0;
        const auto r = std::from_chars(kv.first.data(), kv.first.data() + kv.first.size(), fid);
        if (kv.first.empty() || r.ec != std::errc() || r.ptr != kv.first.data() + kv.first.size()) fail_str("Normalizer: bad feature id " + kv.first);
        if (!kv.second.is_object()) fail_str("Normalizer: feature " + kv.first + " has no record");
        ComputedStats cs;
        const Value* n = kv.second.find("num_elements");
        if (!n || n->kind != Value::UInt) fail_str("Normalizer: feature " + kv.first + " has no count num_elements");
        cs.num_elements = n->u;
        cs.mean = norm_json_stat(kv.second, "mean", kv.first), cs.variance = norm_json_stat(kv.second, "variance", kv.first);
        cs.max = norm_json_stat(kv.second, "max", kv.first), cs.min = norm_json_stat(kv.second, "min", kv.first);
        cs.total = norm_json_stat(kv.second, "total", kv.first);
        nm.stats[fid] = cs;
    }
    return nm;
}

// what normalize_apply_kernel does to each of the d columns (src/normalizers.rs:55-108; a feature without a record keeps
// its values)
inline std::vector<frdev::NormParam> norm_params(const Normalizer& nm, size_t d) {
    std::vector<frdev::NormParam> out(d, frdev::NormParam{0.0f, 0.0f, frdev::NORM_KEEP});
    if (nm.kind == Normalizer::Sigmoid) {
        for (auto& p : out) p.kind = frdev::NORM_SIGMOID;
        return out;
    }
    for (const auto& kv : nm.stats) {
        if (kv.first >= d) continue;
        out[kv.first] = nm.kind == Normalizer::MaxMin ? frdev::norm_param_maxmin(kv.second.max, kv.second.min)
                                                      : frdev::norm_param_zscore(kv.second.mean, (float)std::sqrt(kv.second.variance));
    }
    return out;
}

}  // namespace fr
