// Host half of the device text parser ("Text loading"): what turns the device's per-line records, its matrix
// and its presence bits into exactly the dataset load_ranksvm builds.  No HIP in here -- tests/ranksvm_merge_sanitize.cpp
// runs this header alone under ASan + UBSan on hand-made records.
//
//   merge_lines   after pass 1: parses the lines the device flagged with parse_ranksvm_line in ascending line order (the
//                 first that raises is the file's error: every line that can raise is flagged by construction), interns the
//                 queries in first-appearance order, takes docids from the comment spans, fixes d = 1 + max fid.
//   merge_finish  after pass 2: writes the host-parsed rows into the matrix and the presence bits the device left zero
//                 there, and lists the features present.
#pragma once
#include <cstring>
#include <map>
#include <unordered_map>

#include "ranksvm_line.hpp"
#include "text_number.hpp"

namespace frtext {

// pass 1's record of one line; spans are byte offsets from the line's start
struct TextLineRec {
    uint32_t reason;  // Reason; R_NONE: the device parses this line
    float label;
    uint32_t qid_off, qid_len;  // after "qid:"
    uint32_t com_off, com_len;  // the trimmed comment
    uint32_t has_hash;
    uint32_t count, max_fid;    // features on the line, the largest id
};
static_assert(sizeof(TextLineRec) == 36, "downloaded as it is");

struct MergedText {
    size_t n = 0, d = 0;
    std::vector<float> x;  // n x d
    std::vector<float> gain;
    std::vector<uint32_t> qix;
    std::vector<std::string> qnames, docids;
    std::vector<uint8_t> doc_present;
    std::vector<uint32_t> features;
    std::vector<uint32_t> present_bits;
    size_t present_words = 0;
    bool has_docids = false;
};

struct TextMergePlan {
    size_t n = 0, d = 0;
    bool any_absent = false;       // some row holds fewer than d features: present_bits are kept
    uint32_t dense_len_max = 0;    // the longest dense row: features 0 .. dense_len_max - 1 are present
    bool device_sparse = false;    // a device-parsed row is sparse: the device's per-feature bits matter
    std::vector<uint64_t> host_lines;       // line indices (0-based) the host parsed, ascending
    std::vector<fr::RanksvmLine> host_rows;  // their rows
    uint64_t reasons[R_COUNT] = {0, 0, 0, 0, 0, 0, 0};
};

inline bool row_is_dense(uint32_t count, uint32_t max_fid) { return (double)count / (double)max_fid >= 0.5; }

// starts[i] .. starts[i + 1] - 1 is line i without its '\n' (starts[n] is one past the text when the last line has none)
inline TextMergePlan merge_lines(const char* text, const uint64_t* starts, size_t n, const TextLineRec* recs, MergedText* out) {
    TextMergePlan pl;
    pl.n = n;
    if (n == 0) throw fr::RanksvmLineError{"No features defined!"};
    for (size_t i = 0; i < n; i++) {
        if (recs[i].reason == R_NONE) continue;
        pl.reasons[recs[i].reason < R_COUNT ? recs[i].reason : R_GRAMMAR]++;
        const std::string line(text + starts[i], (size_t)(starts[i + 1] - 1 - starts[i]));
        pl.host_rows.push_back(fr::parse_ranksvm_line(line, (uint64_t)i + 1));
        pl.host_lines.push_back(i);
    }
    out->n = n;
    out->gain.resize(n), out->qix.resize(n), out->docids.resize(n), out->doc_present.resize(n);
    std::unordered_map<std::string, uint32_t> qslot;
    uint32_t max_fid = 0;
    size_t h = 0;
    std::vector<size_t> held(n);
    std::string qid;
    for (size_t i = 0; i < n; i++) {
        const bool host = h < pl.host_lines.size() && pl.host_lines[h] == i;
        bool has_comment;
        if (host) {
            const fr::RanksvmLine& r = pl.host_rows[h++];
            qid = r.qid, out->gain[i] = r.label, out->docids[i] = r.comment, has_comment = r.has_comment;
            max_fid = std::max(max_fid, r.max_feature);
            pl.dense_len_max = std::max(pl.dense_len_max, r.dense_len);
            held[i] = r.dense_len > 0 ? r.dense_len : r.feats.size();
        } else {
            const TextLineRec& r = recs[i];
            const char* s = text + starts[i];
            qid.assign(s + r.qid_off, r.qid_len), out->gain[i] = r.label, has_comment = r.has_hash != 0;
            if (has_comment) out->docids[i].assign(s + r.com_off, r.com_len);
            max_fid = std::max(max_fid, r.max_fid);
            const bool dense = row_is_dense(r.count, r.max_fid);
            if (dense) pl.dense_len_max = std::max(pl.dense_len_max, r.max_fid + 1);
            else pl.device_sparse = true;
            held[i] = dense ? (size_t)r.max_fid + 1 : r.count;
        }
        auto it = qslot.find(qid);
        if (it == qslot.end()) {
            it = qslot.emplace(qid, (uint32_t)out->qnames.size()).first;
            out->qnames.push_back(qid);
        }
        out->qix[i] = it->second;
        out->doc_present[i] = has_comment ? 1 : 0;
        out->has_docids = out->has_docids || has_comment;
    }
    pl.d = out->d = (size_t)max_fid + 1;
    for (size_t i = 0; i < n; i++) pl.any_absent = pl.any_absent || held[i] != pl.d;
    out->present_words = pl.any_absent ? (pl.d + 31) / 32 : 0;
    return pl;
}

// out->x holds n x d values (zero in the host-parsed rows), out->present_bits n x present_words words when rows lack
// features (else it is empty); feature_bits: (d + 31) / 32 words, the fids of the device's sparse rows (null: none)
inline void merge_finish(const TextMergePlan& pl, const uint32_t* feature_bits, MergedText* out) {
    const size_t d = pl.d, pw = out->present_words;
    std::vector<uint32_t> feat((d + 31) / 32, 0u);
    if (feature_bits && pl.device_sparse) std::memcpy(feat.data(), feature_bits, feat.size() * sizeof(uint32_t));
    for (size_t h = 0; h < pl.host_lines.size(); h++) {
        const size_t i = (size_t)pl.host_lines[h];
        const fr::RanksvmLine& r = pl.host_rows[h];
        for (const auto& fv : r.feats) out->x[i * d + fv.first] = fv.second;
        uint32_t* b = pw ? out->present_bits.data() + i * pw : nullptr;
        if (r.dense_len > 0) {
            for (uint32_t j = 0; b && j < r.dense_len; j++) b[j >> 5] |= 1u << (j & 31);
        } else {
            for (const auto& fv : r.feats) {
                feat[fv.first >> 5] |= 1u << (fv.first & 31);
                if (b) b[fv.first >> 5] |= 1u << (fv.first & 31);
            }
        }
    }
    for (uint32_t j = 0; j < pl.dense_len_max; j++) out->features.push_back(j);
    for (size_t j = pl.dense_len_max; j < d; j++)
        if (feat[j >> 5] >> (j & 31) & 1u) out->features.push_back((uint32_t)j);
}

}  // namespace frtext
