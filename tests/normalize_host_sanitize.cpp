// A program of its own over csrc/normalize_host.hpp (the record, its push and fold, the finishing, the per-value functions
// and the wire form of DESIGN.md section 14), for -fsanitize=address,undefined: empty chunks, a feature held nowhere, a fold
// of one record, malformed JSON.  tests/test_normalize_host.py builds and runs it.
#include <cstdio>
#include <cstring>

#include "normalize_host.hpp"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static bool refused(const char* text, const char* needle) {
    try {
        fr::norm_from_json(frjson::parse(text));
    } catch (const fr::FrError& e) {
        return e.debug.find(needle) != std::string::npos;
    } catch (const frjson::ParseError&) {
        return std::strcmp(needle, "parse") == 0;
    }
    return false;
}

int main() {
    // the reference's own known answer (src/stats.rs:178-190)
    const float known[4] = {0.0f, 1.0f, 1.0f, 0.0f};
    fr::ComputedStats cs;
    CHECK(fr::norm_finish(fr::norm_chunked(known, nullptr, 4), &cs));
    CHECK(cs.num_elements == 4 && cs.mean == 0.5 && cs.variance == 1.0 / 3.0 && cs.max == 1.0 && cs.min == 0.0 && cs.total == 2.0);

    // 700 instances: chunk 0 holds the feature, chunk 1 not at all (an empty record in the middle), chunk 2 one value
    std::vector<float> vals(700);
    std::vector<uint8_t> held(700, 0);
    for (size_t i = 0; i < vals.size(); i++) vals[i] = (float)(i % 7) - 3.0f;
    for (size_t i = 0; i < 256; i += 3) held[i] = 1;
    held[699] = 1;
    const frdev::NormRecord r = fr::norm_chunked(vals.data(), held.data(), vals.size());
    CHECK(r.n == 86 + 1 && r.max == 3.0 && r.min == -3.0);
    // a feature held nowhere: no record, whatever the list's length (none at all too)
    std::fill(held.begin(), held.end(), 0);
    CHECK(!fr::norm_finish(fr::norm_chunked(vals.data(), held.data(), vals.size()), &cs));
    CHECK(!fr::norm_finish(fr::norm_chunked(vals.data(), held.data(), 0), &cs));
    held[300] = 1;  // one value: still none
    CHECK(!fr::norm_finish(fr::norm_chunked(vals.data(), held.data(), vals.size()), &cs));
    // a fold of one record is that record, bit for bit
    frdev::NormRecord one = frdev::norm_empty();
    for (int i = 0; i < 5; i++) frdev::norm_push(one, 0.1 * i);
    frdev::NormRecord acc = frdev::norm_empty();
    frdev::norm_fold(acc, frdev::norm_empty());
    frdev::norm_fold(acc, one);
    frdev::norm_fold(acc, frdev::norm_empty());
    CHECK(std::memcmp(&acc, &one, sizeof(one)) == 0);

    // the per-value functions
    fr::Normalizer nm;
    nm.kind = fr::Normalizer::MaxMin;
    nm.stats[1] = fr::ComputedStats{4, 0.5, 1.0 / 3.0, 1.0, 0.0, 2.0};
    nm.stats[2] = fr::ComputedStats{4, 7.0, 0.0, 7.0, 7.0, 28.0};
    nm.stats[9] = fr::ComputedStats{4, 7.0, 0.0, 8.0, 7.0, 28.0};  // past the matrix: ignored
    std::vector<frdev::NormParam> p = fr::norm_params(nm, 3);
    CHECK(p.size() == 3 && p[0].kind == frdev::NORM_KEEP && p[1].kind == frdev::NORM_AFFINE && p[2].kind == frdev::NORM_ZERO);
    CHECK(frdev::norm_affine(0.25f, p[1]) == 0.25f);
    nm.kind = fr::Normalizer::ZScore;
    p = fr::norm_params(nm, 3);
    CHECK(p[1].kind == frdev::NORM_AFFINE && p[1].a == 0.5f && p[1].b == (float)std::sqrt(1.0 / 3.0) && p[2].kind == frdev::NORM_ZERO);

    // the wire form: a round trip, `linear` is MaxMinNormalizer, the refusals
    const std::string text = frjson::dump(fr::norm_to_json(nm));
    const fr::Normalizer back = fr::norm_from_json(frjson::parse(text.c_str()));
    CHECK(back.kind == fr::Normalizer::ZScore && back.stats.size() == 3 && back.stats.at(1).variance == 1.0 / 3.0 && back.stats.at(9).max == 8.0);
    CHECK(frjson::dump(fr::norm_to_json(back)) == text);
    nm.kind = fr::norm_method("linear");
    CHECK(nm.kind == fr::Normalizer::MaxMin && fr::norm_to_json(nm).obj[0].first == "MaxMinNormalizer");
    CHECK(fr::norm_from_json(frjson::parse("{\"PerQuery\": \"linear\"}")).kind == fr::Normalizer::PerQueryMaxMin);
    CHECK(fr::norm_from_json(frjson::parse("{\"SigmoidNormalizer\": []}")).kind == fr::Normalizer::Sigmoid);
    CHECK(refused("{\"RobustNormalizer\": {}}", "Unsupported Normalizer: RobustNormalizer"));
    CHECK(refused("{\"PerQuery\": \"sigmoid\"}", "Unsupported Normalizer: sigmoid"));
    CHECK(refused("{\"PerQuery\": \"robust\"}", "Unsupported Normalizer: robust"));
    CHECK(refused("{\"PerQuery\": 3}", "Unsupported Normalizer"));
    CHECK(refused("[]", "Unsupported Normalizer"));
    CHECK(refused("{}", "Unsupported Normalizer"));
    CHECK(refused("{\"ZScoreNormalizer\": {}}", "feature_stats"));
    CHECK(refused("{\"ZScoreNormalizer\": {\"feature_stats\": {\"x\": {}}}}", "bad feature id"));
    CHECK(refused("{\"ZScoreNormalizer\": {\"feature_stats\": {\"1\": 4}}}", "has no record"));
    CHECK(refused("{\"ZScoreNormalizer\": {\"feature_stats\": {\"1\": {\"num_elements\": -2}}}}", "num_elements"));
    CHECK(refused("{\"ZScoreNormalizer\": {\"feature_stats\": {\"1\": {\"num_elements\": 2, \"mean\": null}}}}", "no finite number for mean"));
    CHECK(refused("{\"ZScoreNormalizer\": {\"feature_stats\": {\"1\": {\"num_elements\": 2, \"mean\": 1e999}}}}", "parse"));
    CHECK(refused("{\"ZScoreNormalizer\": {\"feature_stats\": {\"1\": {\"num_elements\": 2, \"mean\": NaN}}}}", "parse"));
    CHECK(refused("{\"ZScoreNormalizer\": {\"feature_stats\": ", "parse"));
    bool bad_method = false;
    try {
        fr::norm_method("robust");
    } catch (const fr::FrError& e) {
        bad_method = e.debug.find("Unsupported Normalizer: robust") != std::string::npos;
    }
    CHECK(bad_method);
    std::printf("normalize_host ok\n");
    return 0;
}
