// One line of a ranksvm / libsvm feature file (src/libsvm.rs:131-189, src/instance.rs:104-130): label, qid, features, the
// sort and duplicate check, the dense-or-sparse rule.  The host parser (loader.hpp) calls it for every line, the device
// parser's merge (text_merge.hpp) for the lines the device declined.  Standard library only.
#pragma once
#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

namespace fr {

inline std::vector<std::string> split_ws(const std::string& s) {
    std::vector<std::string> out;
    size_t i = 0, n = s.size();
    while (i < n) {
        while (i < n && isspace((unsigned char)s[i])) i++;
        size_t j = i;
        while (j < n && !isspace((unsigned char)s[j])) j++;
        if (j > i) out.emplace_back(s, i, j - i);
        i = j;
    }
    return out;
}

inline std::string trim(const std::string& s) {
    size_t a = 0, b = s.size();
    while (a < b && isspace((unsigned char)s[a])) a++;
    while (b > a && isspace((unsigned char)s[b - 1])) b--;
    return s.substr(a, b - a);
}

inline bool parse_f64_strict(const std::string& t, double* out) {
    if (t.empty()) return false;
    char* end = nullptr;
    *out = strtod(t.c_str(), &end);
    return end == t.c_str() + t.size();
}
inline bool parse_f32_strict(const std::string& t, float* out) {
    if (t.empty()) return false;
    char* end = nullptr;
    *out = strtof(t.c_str(), &end);  // correctly rounded, like fast_float::parse::<f32>
    return end == t.c_str() + t.size();
}

// What a line's error says after "<path>: " (LineParseError(<line>, <kind>) or "Missing qid").
struct RanksvmLineError {
    std::string what;
};

struct RanksvmLine {
    float label = 0.0f;
    std::string qid, comment;
    bool has_comment = false;
    std::vector<std::pair<uint32_t, float>> feats;  // ascending by feature id
    uint32_t max_feature = 0;
    uint32_t dense_len = 0;  // >0: Dense32 of this length (instance.rs:108-115)
};

inline RanksvmLine parse_ranksvm_line(const std::string& line, uint64_t line_no) {
    auto lerr = [&](const std::string& kind) { throw RanksvmLineError{"LineParseError(" + std::to_string(line_no) + ", " + kind + ")"}; };
    RanksvmLine row;
    std::string data = line;
    size_t hash = line.find('#');
    if (hash != std::string::npos) {
        data = line.substr(0, hash);
        row.comment = trim(line.substr(hash + 1));
        row.has_comment = true;
    }
    std::vector<std::string> toks = split_ws(data);
    if (toks.empty()) lerr("EmptyLine");
    double label64;
    if (!parse_f64_strict(toks[0], &label64)) lerr("Label(ParseFloatError { kind: Invalid })");
    row.label = (float)label64;
    if (row.label != row.label) lerr("LabelIsNan(FloatIsNan)");
    size_t t = 1;
    bool has_q = false;
    if (t < toks.size() && toks[t].compare(0, 4, "qid:") == 0) {
        row.qid = toks[t];
        while (row.qid.compare(0, 4, "qid:") == 0) row.qid.erase(0, 4);  // trim_start_matches
        has_q = true;
        t++;
    }
    for (; t < toks.size(); t++) {
        size_t colon = toks[t].find(':');
        if (colon == std::string::npos) lerr("FeatureNoColon");
        std::string fs = toks[t].substr(0, colon), vs = toks[t].substr(colon + 1);
        char* end = nullptr;
        unsigned long long fid = strtoull(fs.c_str(), &end, 10);
        if (fs.empty() || end != fs.c_str() + fs.size() || fid > 0xFFFFFFFFull || fs[0] == '-')
            lerr("FeatureNum(ParseIntError { kind: InvalidDigit })");
        float val;
        if (!parse_f32_strict(vs, &val)) lerr("FeatureValNotFloat(Error)");
        row.feats.emplace_back((uint32_t)fid, val);
    }
    if (row.feats.empty()) lerr("NoFeatures");
    bool needs_sort = false;
    for (size_t k = 0; k + 1 < row.feats.size(); k++)
        if (row.feats[k].first >= row.feats[k + 1].first) needs_sort = true;
    if (needs_sort) {
        std::sort(row.feats.begin(), row.feats.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (size_t k = 0; k + 1 < row.feats.size(); k++)
            if (row.feats[k].first == row.feats[k + 1].first)
                lerr("MultipleDefinitions(Feature { idx: " + std::to_string(row.feats[k].first) + " })");
    }
    if (!has_q) throw RanksvmLineError{"\"Missing qid\""};
    // instance.rs:104-130: dense when len / max_feature >= 0.5
    for (const auto& fv : row.feats) row.max_feature = std::max(row.max_feature, fv.first);
    double density = (double)row.feats.size() / (double)row.max_feature;
    if (density >= 0.5) row.dense_len = row.max_feature + 1;
    return row;
}

}  // namespace fr
