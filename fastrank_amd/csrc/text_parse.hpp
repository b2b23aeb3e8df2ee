// Interface between the loader (loader.hpp, compiled into capi.o) and the device text parser (text_parse.inc +
// kernels_text.inc, compiled into device.o).  DESIGN.md, "Text loading".
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "text_merge.hpp"

namespace frdev {

constexpr uint32_t TEXT_SCAN_SLICE = 4096;    // bytes of text a wave counts newlines in
constexpr uint32_t TEXT_STAGE_LIMIT = 16384;  // the longest line (without its '\n') a wave stages into LDS

struct TextTimes {
    double upload = 0, line_scan = 0, pass1 = 0, pass2 = 0, download = 0;  // wall seconds
};

// One file's text on the device between the two passes.  Every call returns false on a HIP error (*err); *fits = false
// (with the call returning true) says the device lacks the memory, and the caller falls back to the host parser.
class TextParser {
  public:
    TextParser();
    ~TextParser();
    // uploads the text, finds the lines and runs pass 1: starts[n + 1] (text_merge.hpp: merge_lines), recs[n]
    bool pass1(const char* text, size_t bytes, std::vector<uint64_t>* starts, std::vector<frtext::TextLineRec>* recs, bool* fits, TextTimes* t,
               std::string* err);
    // parses the unflagged lines again into x[n * d]; present_bits[n * present_words] when present_words > 0;
    // feature_bits[(d + 31) / 32] (the fids of sparse rows) when feature_bits is not null
    bool pass2(size_t d, size_t present_words, float* x, uint32_t* present_bits, uint32_t* feature_bits, bool* fits, TextTimes* t, std::string* err);

  private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

}  // namespace frdev
