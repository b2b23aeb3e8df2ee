// csrc/text_merge.hpp alone, under -fsanitize=address,undefined (tests/test_ranksvm_parser_host.py builds and runs this):
// hand-made pass-1 records -- flagged lines among unflagged ones, an error on a flagged line after valid flagged lines, two
// error lines, an empty file -- merged, and held to the merge of the same text with every line flagged (the host parser's
// result by construction).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "text_merge.hpp"

using namespace frtext;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

struct Text {
    std::string text;
    std::vector<uint64_t> starts;
    std::vector<std::string> lines;
};

static Text make_text(const std::vector<std::string>& lines, bool final_newline) {
    Text t;
    t.lines = lines;
    for (size_t i = 0; i < lines.size(); i++) {
        t.starts.push_back(t.text.size());
        t.text += lines[i];
        if (i + 1 < lines.size() || final_newline) t.text += '\n';
    }
    t.starts.push_back(t.text.size() + (final_newline ? 0 : 1));
    return t;
}

// what pass 1 writes for a line inside the fast grammar (spans found by hand here, values by the host's own parse)
static TextLineRec device_rec(const std::string& line) {
    TextLineRec r = {};
    const fr::RanksvmLine p = fr::parse_ranksvm_line(line, 1);
    r.reason = R_NONE;
    r.label = p.label;
    r.qid_off = (uint32_t)line.find("qid:") + 4;
    r.qid_len = (uint32_t)p.qid.size();
    const size_t hash = line.find('#');
    if (hash != std::string::npos) {
        r.has_hash = 1;
        size_t a = hash + 1, b = line.size();
        while (a < b && is_space((unsigned char)line[a])) a++;
        while (b > a && is_space((unsigned char)line[b - 1])) b--;
        r.com_off = (uint32_t)a, r.com_len = (uint32_t)(b - a);
    }
    r.count = (uint32_t)p.feats.size();
    r.max_fid = p.max_feature;
    return r;
}

struct Result {
    MergedText mt;
    TextMergePlan plan;
    std::string error;
};

// the merge of `t` with the lines of `flagged` handed to the host; the device's share of x / bits / feature bits is made here
static Result run(const Text& t, const std::vector<bool>& flagged) {
    Result out;
    const size_t n = t.lines.size();
    std::vector<TextLineRec> recs(n);
    for (size_t i = 0; i < n; i++) {
        if (flagged[i]) recs[i] = TextLineRec{}, recs[i].reason = R_GRAMMAR + (uint32_t)(i % 3);
        else recs[i] = device_rec(t.lines[i]);
    }
    try {
        out.plan = merge_lines(t.text.data(), t.starts.data(), n, recs.data(), &out.mt);
    } catch (const fr::RanksvmLineError& e) {
        out.error = e.what;
        return out;
    }
    MergedText& mt = out.mt;
    const size_t d = mt.d, pw = mt.present_words;
    mt.x.assign(n * d, 0.0f);
    if (pw) mt.present_bits.assign(n * pw, 0u);
    std::vector<uint32_t> fbits((d + 31) / 32, 0u);
    for (size_t i = 0; i < n; i++) {
        if (flagged[i]) continue;
        const fr::RanksvmLine p = fr::parse_ranksvm_line(t.lines[i], i + 1);
        for (const auto& fv : p.feats) {
            mt.x[i * d + fv.first] = fv.second;
            if (p.dense_len == 0) {
                fbits[fv.first >> 5] |= 1u << (fv.first & 31);
                if (pw) mt.present_bits[i * pw + (fv.first >> 5)] |= 1u << (fv.first & 31);
            }
        }
        for (uint32_t j = 0; pw && j < p.dense_len; j++) mt.present_bits[i * pw + (j >> 5)] |= 1u << (j & 31);
    }
    merge_finish(out.plan, out.plan.device_sparse ? fbits.data() : nullptr, &mt);
    return out;
}

static void same(const MergedText& a, const MergedText& b) {
    CHECK(a.n == b.n && a.d == b.d && a.present_words == b.present_words && a.has_docids == b.has_docids);
    CHECK(a.x.size() == b.x.size() && std::memcmp(a.x.data(), b.x.data(), a.x.size() * sizeof(float)) == 0);
    CHECK(a.gain.size() == b.gain.size() && std::memcmp(a.gain.data(), b.gain.data(), a.gain.size() * sizeof(float)) == 0);
    CHECK(a.qix == b.qix && a.qnames == b.qnames && a.docids == b.docids && a.doc_present == b.doc_present);
    CHECK(a.features == b.features && a.present_bits == b.present_bits);
}

int main() {
    const std::vector<std::string> lines = {
        "2 qid:7 1:0.5 2:1.5 3:-0 # doc a ",  // dense
        "0 qid:7 3:1e5 1:2 # doc b",          // unsorted: the host's
        "1 qid:8 40:16777217",                // sparse, a near tie: the host's
        "0 qid:7 33:4 64:5 #",                // sparse, an empty comment, d = 65
        "1 qid:qid:9 0:1 1:2\r",              // qid:qid: is the host's (strips both)
        "3 qid:8 1:1 2:2 3:3 4:4 5:5 6:6",    // dense
    };
    const std::vector<bool> mask_all(lines.size(), true), mask_some = {false, true, true, false, true, false};
    for (int final_newline = 0; final_newline < 2; final_newline++) {
        const Text t = make_text(lines, final_newline != 0);
        const Result all = run(t, mask_all), some = run(t, mask_some);
        CHECK(all.error.empty() && some.error.empty());
        same(all.mt, some.mt);
        CHECK(some.mt.n == 6 && some.mt.d == 65 && some.mt.present_words == 3 && some.plan.host_lines.size() == 3);
        CHECK(some.mt.qnames == (std::vector<std::string>{"7", "8", "9"}) && some.mt.qix == (std::vector<uint32_t>{0, 0, 1, 0, 2, 1}));
        CHECK(some.mt.docids[0] == "doc a" && some.mt.docids[3].empty() && some.mt.doc_present[3] == 1 && some.mt.doc_present[2] == 0);
        CHECK(some.mt.features == (std::vector<uint32_t>{0, 1, 2, 3, 4, 5, 6, 33, 40, 64}));
        CHECK(some.mt.x[1 * 65 + 3] == 1e5f && some.mt.x[2 * 65 + 40] == 16777216.0f && std::signbit(some.mt.x[3]));
        CHECK(some.plan.reasons[R_GRAMMAR] + some.plan.reasons[R_NUMBER] + some.plan.reasons[R_UNSORTED] == 3);
    }
    {   // every row holds every feature: no presence bits are kept
        const Text t = make_text({"1 qid:1 0:1 1:2", "0 qid:1 1:5 0:4"}, true);
        const Result r = run(t, {false, true}), all = run(t, {true, true});
        same(r.mt, all.mt);
        CHECK(r.mt.present_words == 0 && r.mt.present_bits.empty() && r.mt.d == 2 && r.mt.x[2] == 4.0f && r.mt.x[3] == 5.0f);
    }
    {   // an error on a flagged line after valid flagged lines; of two error lines the first is the file's
        const Text t = make_text({"1 qid:1 1:1", "1 qid:1 2:1 1:3", "1 qid:1 1:x", "1 qid:1 1:1", "zz qid:1 1:1", "1 1:1"}, true);
        const Result r = run(t, {false, true, true, false, true, true});
        CHECK(r.error == "LineParseError(3, FeatureValNotFloat(Error))");
        const Text u = make_text({"1 qid:1 1:1", "1 1:2", ""}, false);
        CHECK(run(u, {false, true, true}).error == "\"Missing qid\"");
        const Text v = make_text({"1 qid:1 1:1", "", "1 1:2"}, true);
        CHECK(run(v, {false, true, true}).error == "LineParseError(2, EmptyLine)");
        const Text w = make_text({"1 qid:1 4:1 4:2"}, true);
        CHECK(run(w, {true}).error == "LineParseError(1, MultipleDefinitions(Feature { idx: 4 }))");
    }
    {   // an empty file
        const Text t = make_text({}, true);
        CHECK(run(t, {}).error == "No features defined!");
    }
    std::printf("ranksvm_merge ok\n");
    return 0;
}
