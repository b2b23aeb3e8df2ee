// Text loaders that feed the device path: ranksvm/libsvm feature files and TREC qrels.
// Behaviour follows src/libsvm.rs:131-189, src/instance.rs:104-130, src/dataset.rs:211-256 and
// src/qrel.rs:65-102.  Every loaded dataset is densified to an n x n_dim f32 matrix (a missing
// feature reads 0.0, exactly what Features::get -> None -> unwrap_or(0.0) and the sparse dot
// product give) so that it runs through the same HIP kernels as a numpy-made DenseDataset.
#pragma once
#include <zlib.h>

#include <cstdlib>
#include <cstring>

#include "host.hpp"
#include "ranksvm_line.hpp"
#include "text_parse.hpp"

namespace fr {

// io_helper.rs:18-34 sniffs .gz/.bz2/.zst; zlib's gz* API reads both plain and gzip streams.
class LineReader {
  public:
    explicit LineReader(const std::string& path) {
        auto ends = [&](const char* suf) {
            size_t n = strlen(suf);
            return path.size() >= n && path.compare(path.size() - n, n, suf) == 0;
        };
        if (ends(".bz2") || ends(".zst"))
            fail_str(path + ": bzip2/zstd inputs are not supported by the MI355X build (use .gz or plain text)");
        f_ = gzopen(path.c_str(), "rb");
        if (!f_) {
            fail_raw("Os { code: " + std::to_string(errno) + ", kind: " + (errno == ENOENT ? "NotFound" : "Other") +
                     ", message: " + frjson::rust_debug_str(strerror(errno)) + " }");
        }
        gzbuffer(f_, 1 << 20);
    }
    ~LineReader() {
        if (f_) gzclose(f_);
    }
    bool next(std::string& line) {
        line.clear();
        char buf[1 << 16];
        bool got = false;
        while (gzgets(f_, buf, sizeof(buf))) {
            got = true;
            size_t len = strlen(buf);
            line.append(buf, len);
            if (len && buf[len - 1] == '\n') break;
        }
        return got;
    }

  private:
    gzFile f_ = nullptr;
};

// (split_ws, trim, parse_f64_strict, parse_f32_strict: ranksvm_line.hpp)

// dataset.rs:14-25 load_feature_names_json: {"1": "name", ...}
inline std::map<uint32_t, std::string> load_feature_names(const std::string& path) {
    LineReader rd(path);
    std::string text, line;
    while (rd.next(line)) text += line;
    Value v;
    try {
        v = frjson::parse(text.c_str());
    } catch (const frjson::ParseError& e) {
        fail_raw(e.debug());
    }
    if (!v.is_object()) fail_raw("Error(\"invalid type: expected a map\", line: 1, column: 1)");
    std::map<uint32_t, std::string> out;
    for (const auto& m : v.obj) {
        char* end = nullptr;
        unsigned long long k = strtoull(m.first.c_str(), &end, 10);
        if (m.first.empty() || end != m.first.c_str() + m.first.size())
            fail_raw("ParseIntError { kind: InvalidDigit }");
        if (!m.second.is_string()) fail_raw("Error(\"invalid type: expected a string\", line: 1, column: 1)");
        out[(uint32_t)k] = m.second.s;
    }
    return out;
}

// What the last open of a feature file did (fr_last_load_stats).
struct LoadStats {
    std::string parser = "host", reason;
    uint64_t bytes = 0, lines = 0, host_lines = 0;
    uint64_t reasons[frtext::R_COUNT] = {0, 0, 0, 0, 0, 0, 0};  // host_lines by frtext::Reason
    double read = 0, merge = 0, total = 0;                      // wall seconds; the device's stages in `dev`
    frdev::TextTimes dev;
};

// The (inflated) text from which parser = "auto" takes the device parser when a device is present.  A condition, not a
// tuning result: DESIGN.md ("Text loading") has the measured crossover, which lies below it.
constexpr size_t TEXT_DEVICE_THRESHOLD = size_t(32) << 20;

inline std::shared_ptr<DatasetView> view_of_core(const std::shared_ptr<DataCore>& core, const std::map<uint32_t, std::string>* names) {
    if (names) core->feature_names = *names;
    auto view = std::make_shared<DatasetView>();
    view->core = core;
    view->features = core->features;
    view->instances.resize(core->n);
    for (size_t i = 0; i < core->n; i++) view->instances[i] = (uint32_t)i;
    return view;
}

inline std::shared_ptr<DatasetView> load_ranksvm(const std::string& path, const std::map<uint32_t, std::string>* names,
                                                 LoadStats* stats = nullptr) {
    struct Row {
        std::vector<std::pair<uint32_t, float>> feats;
        uint32_t dense_len = 0;  // >0: Dense32 of this length (instance.rs:108-115)
    };
    auto core = std::make_shared<DataCore>();
    std::vector<Row> rows;
    std::unordered_map<std::string, uint32_t> qslot;
    std::set<uint32_t> present;
    bool any_docid = false;
    {
        LineReader rd(path);
        std::string line;
        uint64_t line_no = 0;
        while (rd.next(line)) {
            line_no++;
            if (stats) stats->bytes += line.size(), stats->lines = line_no;
            RanksvmLine parsed;
            try {
                parsed = parse_ranksvm_line(line, line_no);
            } catch (const RanksvmLineError& e) {
                fail_str(path + ": " + e.what);
            }
            Row row;
            row.feats = std::move(parsed.feats);
            row.dense_len = parsed.dense_len;
            if (row.dense_len > 0) {
                for (uint32_t j = 0; j < row.dense_len; j++) present.insert(j);
            } else {
                for (const auto& fv : row.feats) present.insert(fv.first);
            }
            auto it = qslot.find(parsed.qid);
            if (it == qslot.end()) {
                it = qslot.emplace(parsed.qid, (uint32_t)core->qnames.size()).first;
                core->qnames.push_back(parsed.qid);
            }
            core->qix.push_back(it->second);
            core->gain.push_back(parsed.label);
            core->docids.push_back(parsed.comment);
            core->doc_present.push_back(parsed.has_comment ? 1 : 0);  // document_name() is Some only then
            any_docid = any_docid || parsed.has_comment;
            rows.push_back(std::move(row));
        }
    }
    if (rows.empty() || present.empty()) fail_str(path + ": No features defined!");
    core->n = rows.size();
    core->d = (size_t)(*present.rbegin()) + 1;
    core->features.assign(present.begin(), present.end());
    core->x_own.assign(core->n * core->d, 0.0f);
    for (size_t i = 0; i < rows.size(); i++)
        for (const auto& fv : rows[i].feats) core->x_own[i * core->d + fv.first] = fv.second;
    core->x = core->x_own.data();
    {
        // which features every row holds (see DataCore::present_bits); kept only if some row lacks some feature
        const size_t pw = (core->d + 31) / 32;
        std::vector<uint32_t> bits(core->n * pw, 0u);
        bool any_absent = false;
        for (size_t i = 0; i < rows.size(); i++) {
            uint32_t* b = bits.data() + i * pw;
            size_t held = 0;
            if (rows[i].dense_len > 0) {
                for (uint32_t j = 0; j < rows[i].dense_len && j < core->d; j++) b[j >> 5] |= 1u << (j & 31), held++;
            } else {
                for (const auto& fv : rows[i].feats) b[fv.first >> 5] |= 1u << (fv.first & 31), held++;
            }
            any_absent = any_absent || held != core->d;
        }
        if (any_absent) {
            core->present_bits = std::move(bits);
            core->present_words = pw;
        }
    }
    core->has_docids = any_docid;
    return view_of_core(core, names);
}

// The file whole, inflated through zlib as LineReader reads it (same refusals, same error for a file that does not open).
inline std::vector<char> read_text_whole(const std::string& path) {
    auto ends = [&](const char* suf) {
        size_t n = strlen(suf);
        return path.size() >= n && path.compare(path.size() - n, n, suf) == 0;
    };
    if (ends(".bz2") || ends(".zst"))
        fail_str(path + ": bzip2/zstd inputs are not supported by the MI355X build (use .gz or plain text)");
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) {
        fail_raw("Os { code: " + std::to_string(errno) + ", kind: " + (errno == ENOENT ? "NotFound" : "Other") +
                 ", message: " + frjson::rust_debug_str(strerror(errno)) + " }");
    }
    gzbuffer(f, 1 << 20);
    std::vector<char> text;
    size_t used = 0;
    for (;;) {
        if (text.size() - used < (size_t(1) << 24)) text.resize(std::max<size_t>(text.size() * 2, size_t(1) << 25));
        const int got = gzread(f, text.data() + used, (unsigned)std::min<size_t>(text.size() - used, size_t(1) << 30));
        if (got <= 0) break;
        used += (size_t)got;
    }
    gzclose(f);
    text.resize(used);
    return text;
}

// The device parser ("Text loading"): text in `text`; nullptr when it hands the file to the host parser
// (stats->reason says why).  Errors are the host parser's, word for word.
inline std::shared_ptr<DatasetView> load_ranksvm_text_device(const std::string& path, const std::vector<char>& text,
                                                             const std::map<uint32_t, std::string>* names, LoadStats* stats) {
    using Clock = std::chrono::steady_clock;
    auto secs = [](Clock::time_point a) { return std::chrono::duration<double>(Clock::now() - a).count(); };
    if (!text.empty() && memchr(text.data(), 0, text.size())) {
        stats->reason = "the text holds a NUL byte";
        return nullptr;
    }
    frdev::TextParser parser;
    std::vector<uint64_t> starts;
    std::vector<frtext::TextLineRec> recs;
    bool fits = true;
    std::string err;
    if (!parser.pass1(text.data(), text.size(), &starts, &recs, &fits, &stats->dev, &err)) fail_str(err);
    if (!fits) {
        stats->reason = "the device lacks the memory for the text and its line tables";
        return nullptr;
    }
    auto t0 = Clock::now();
    frtext::MergedText mt;
    frtext::TextMergePlan plan;
    try {
        plan = frtext::merge_lines(text.data(), starts.data(), recs.size(), recs.data(), &mt);
    } catch (const RanksvmLineError& e) {
        fail_str(path + ": " + e.what);
    }
    mt.x.assign(mt.n * mt.d, 0.0f);
    if (mt.present_words) mt.present_bits.assign(mt.n * mt.present_words, 0u);
    std::vector<uint32_t> feature_bits(plan.device_sparse ? (mt.d + 31) / 32 : 0, 0u);
    stats->merge += secs(t0);
    if (!parser.pass2(mt.d, mt.present_words, mt.x.data(), mt.present_bits.data(), plan.device_sparse ? feature_bits.data() : nullptr, &fits,
                      &stats->dev, &err))
        fail_str(err);
    if (!fits) {
        stats->reason = "the device lacks the memory for the n x d matrix";
        return nullptr;
    }
    t0 = Clock::now();
    frtext::merge_finish(plan, plan.device_sparse ? feature_bits.data() : nullptr, &mt);
    auto core = std::make_shared<DataCore>();
    core->n = mt.n, core->d = mt.d;
    core->x_own = std::move(mt.x);
    core->x = core->x_own.data();
    core->gain = std::move(mt.gain), core->qix = std::move(mt.qix), core->qnames = std::move(mt.qnames);
    core->docids = std::move(mt.docids), core->doc_present = std::move(mt.doc_present), core->has_docids = mt.has_docids;
    core->features = std::move(mt.features);
    core->present_bits = std::move(mt.present_bits), core->present_words = mt.present_words;
    stats->merge += secs(t0);
    stats->lines = mt.n;
    stats->host_lines = plan.host_lines.size();
    for (uint32_t r = 0; r < frtext::R_COUNT; r++) stats->reasons[r] = plan.reasons[r];
    return view_of_core(core, names);
}

// parser: "auto" (the device parser when a device is present and the text is at least TEXT_DEVICE_THRESHOLD), "host", "device"
inline std::shared_ptr<DatasetView> load_ranksvm_with(const std::string& path, const std::map<uint32_t, std::string>* names,
                                                      const std::string& parser, LoadStats* stats) {
    using Clock = std::chrono::steady_clock;
    const auto t0 = Clock::now();
    auto secs = [](Clock::time_point a) { return std::chrono::duration<double>(Clock::now() - a).count(); };
    *stats = LoadStats();
    if (parser != "auto" && parser != "host" && parser != "device")
        fail_str("unknown parser \"" + parser + "\": expected one of \"auto\", \"host\", \"device\"");
    auto host = [&](const std::string& why) {
        LoadStats st;
        st.reason = why, st.read = stats->read, st.dev = stats->dev;
        *stats = st;
        auto view = load_ranksvm(path, names, stats);
        stats->total = secs(t0);
        return view;
    };
    if (parser == "host") return host("parser = host");
    std::string e2;
    const bool have_device = frdev::device_count(&e2) > 0;
    if (!have_device) {
        if (parser == "device")
            fail_str("no MI355X/HIP device available for the fastrank_amd compute path (" + (e2.empty() ? std::string("device count is 0") : e2) + ")");
        return host("no device");
    }
    if (parser == "auto") {
        // a plain file shorter than the threshold is the host's without being read twice; a gzip stream is inflated to find out
        FILE* fh = fopen(path.c_str(), "rb");
        if (fh) {
            unsigned char magic[2] = {0, 0};
            const size_t got = fread(magic, 1, 2, fh);
            const bool gz = got == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
            fseek(fh, 0, SEEK_END);
            const long size = ftell(fh);
            fclose(fh);
            if (!gz && size >= 0 && (size_t)size < TEXT_DEVICE_THRESHOLD) return host("the text is shorter than the threshold");
        }
    }
    const std::vector<char> text = read_text_whole(path);
    stats->read = secs(t0);
    stats->bytes = text.size();
    if (parser == "auto" && text.size() < TEXT_DEVICE_THRESHOLD) return host("the text is shorter than the threshold");
    stats->parser = "device";
    stats->reason = parser == "device" ? "parser = device" : "a device is present and the text reaches the threshold";
    auto view = load_ranksvm_text_device(path, text, names, stats);
    if (!view) return host(stats->reason);
    stats->total = secs(t0);
    return view;
}

// src/qrel.rs:65-102
inline QRel load_qrel_file(const std::string& path) {
    QRel q;
    LineReader rd(path);
    std::string line;
    uint64_t num = 0;
    while (rd.next(line)) {
        num++;
        std::vector<std::string> row = split_ws(line);
        if (row.size() < 4) fail_str(path + ":" + std::to_string(num) + ": expected 4 columns");
        float gain;
        if (!parse_f32_strict(row[3], &gain))
            fail_str(path + ":" + std::to_string(num) + ": Invalid relevance judgment " + row[3]);
        if (gain != gain) fail_str(path + ":" + std::to_string(num) + ": NaN relevance judgment.");
        q.insert(row[0], row[2], gain);
    }
    return q;
}

}  // namespace fr
