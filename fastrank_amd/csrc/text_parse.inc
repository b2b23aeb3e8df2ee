// Launch side of the device text parser (text_parse.hpp; kernels in kernels_text.inc; DESIGN.md, "Text loading").

struct TextParser::Impl {
    DevBuf<unsigned char> text;
    DevBuf<uint32_t> counts;
    DevBuf<uint64_t> offsets, starts;
    DevBuf<unsigned char> temp;
    DevBuf<frtext::TextLineRec> recs;
    DevBuf<float> x;
    DevBuf<uint32_t> pbits, fbits;
    size_t bytes = 0, n = 0;
    int grid = 0;
};

TextParser::TextParser() : impl_(new Impl()) {}
TextParser::~TextParser() {}

namespace {
using TextClock = std::chrono::steady_clock;
inline double text_lap(TextClock::time_point* t0) {
    const auto now = TextClock::now();
    const double s = std::chrono::duration<double>(now - *t0).count();
    *t0 = now;
    return s;
}
// free device memory, with a tenth of it left alone
inline bool text_room(size_t* room, std::string* err) {
    size_t free_b = 0, total_b = 0;
    FR_HIP(hipMemGetInfo(&free_b, &total_b));
    *room = free_b - free_b / 10;
    return true;
}
// the device lacks the memory (by the estimate, or an allocation was refused): not an error, the host parser takes the file
inline bool text_no_room(bool* fits) {
    (void)hipGetLastError();
    *fits = false;
    return true;
}
}  // namespace

bool TextParser::pass1(const char* text, size_t bytes, std::vector<uint64_t>* starts, std::vector<frtext::TextLineRec>* recs, bool* fits,
                       TextTimes* t, std::string* err) {
    Impl& m = *impl_;
    *fits = true;
    starts->clear(), recs->clear();
    m.bytes = bytes, m.n = 0;
    if (bytes == 0) return true;
    auto clock = TextClock::now();
    int dev = 0;
    hipDeviceProp_t prop;
    FR_HIP(hipGetDevice(&dev));
    FR_HIP(hipGetDeviceProperties(&prop, dev));
    m.grid = std::max(1, prop.multiProcessorCount) * 8;
    const size_t nslices = (bytes + TEXT_SCAN_SLICE - 1) / TEXT_SCAN_SLICE;
    const size_t padded = (nslices + 1) * TEXT_SCAN_SLICE;
    size_t room = 0;
    if (!text_room(&room, err)) return false;
    if (padded + nslices * 12 > room) return text_no_room(fits);  // the text and the slice tables
    if (!m.text.ensure(padded, err) || !m.counts.ensure(nslices, err) || !m.offsets.ensure(nslices, err)) return text_no_room(fits);
    FR_HIP(hipMemcpy(m.text.p, text, bytes, hipMemcpyHostToDevice));
    FR_HIP(hipMemset(m.text.p + bytes, 0, padded - bytes));
    FR_HIP(hipDeviceSynchronize());
    t->upload += text_lap(&clock);

    const int scan_grid = (int)std::min<size_t>((nslices + 3) / 4, (size_t)m.grid);
    hipLaunchKernelGGL(text_count_kernel, dim3(scan_grid), dim3(256), 0, nullptr, (const uint4*)m.text.p, (uint64_t)nslices, m.counts.p);
    FR_HIP(hipGetLastError());
    size_t tb = 0;
    FR_HIP(rocprim::exclusive_scan(nullptr, tb, m.counts.p, m.offsets.p, (uint64_t)0, nslices, rocprim::plus<uint64_t>(), nullptr));
    if (!m.temp.ensure(std::max<size_t>(tb, 1), err)) return text_no_room(fits);
    FR_HIP(rocprim::exclusive_scan((void*)m.temp.p, tb, m.counts.p, m.offsets.p, (uint64_t)0, nslices, rocprim::plus<uint64_t>(), nullptr));
    uint64_t last_off = 0;
    uint32_t last_cnt = 0;
    FR_HIP(hipMemcpy(&last_off, m.offsets.p + (nslices - 1), sizeof(last_off), hipMemcpyDeviceToHost));
    FR_HIP(hipMemcpy(&last_cnt, m.counts.p + (nslices - 1), sizeof(last_cnt), hipMemcpyDeviceToHost));
    const uint64_t newlines = last_off + last_cnt;
    const bool open_end = text[bytes - 1] != '\n';  // a last line without '\n' is a line
    const size_t n = (size_t)newlines + (open_end ? 1 : 0);
    m.n = n;
    if (!text_room(&room, err)) return false;
    if ((n + 2) * sizeof(uint64_t) + n * sizeof(frtext::TextLineRec) > room) return text_no_room(fits);
    if (!m.starts.ensure(n + 2, err) || !m.recs.ensure(std::max<size_t>(n, 1), err)) return text_no_room(fits);
    hipLaunchKernelGGL(text_starts_kernel, dim3(scan_grid), dim3(256), 0, nullptr, (const uint4*)m.text.p, (uint64_t)nslices, m.offsets.p, m.starts.p);
    FR_HIP(hipGetLastError());
    const uint64_t first = 0, end_open = (uint64_t)bytes + 1;
    FR_HIP(hipMemcpy(m.starts.p, &first, sizeof(first), hipMemcpyHostToDevice));
    if (open_end) FR_HIP(hipMemcpy(m.starts.p + n, &end_open, sizeof(end_open), hipMemcpyHostToDevice));
    FR_HIP(hipDeviceSynchronize());
    t->line_scan += text_lap(&clock);

    const int grid = (int)std::min<size_t>(n, (size_t)m.grid);
    hipLaunchKernelGGL(text_parse_kernel<1>, dim3(grid), dim3(64), 0, nullptr, (const unsigned char*)m.text.p, (const uint64_t*)m.starts.p, (uint64_t)n,
                       m.recs.p, (float*)nullptr, (uint64_t)0, (uint32_t*)nullptr, (uint64_t)0, (uint32_t*)nullptr);
    FR_HIP(hipGetLastError());
    FR_HIP(hipDeviceSynchronize());
    t->pass1 += text_lap(&clock);

    starts->resize(n + 1), recs->resize(n);
    FR_HIP(hipMemcpy(starts->data(), m.starts.p, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    FR_HIP(hipMemcpy(recs->data(), m.recs.p, n * sizeof(frtext::TextLineRec), hipMemcpyDeviceToHost));
    t->download += text_lap(&clock);
    return true;
}

bool TextParser::pass2(size_t d, size_t present_words, float* x, uint32_t* present_bits, uint32_t* feature_bits, bool* fits, TextTimes* t,
                       std::string* err) {
    Impl& m = *impl_;
    *fits = true;
    const size_t n = m.n, fw = (d + 31) / 32;
    if (n == 0) return true;
    auto clock = TextClock::now();
    size_t room = 0;
    if (!text_room(&room, err)) return false;
    const size_t need_words = n * d + n * present_words + (feature_bits ? fw : 0);
    if (need_words > room / 4) return text_no_room(fits);
    if (!m.x.ensure(n * d, err)) return text_no_room(fits);
    FR_HIP(hipMemset(m.x.p, 0, n * d * sizeof(float)));
    if (present_words) {
        if (!m.pbits.ensure(n * present_words, err)) return text_no_room(fits);
        FR_HIP(hipMemset(m.pbits.p, 0, n * present_words * sizeof(uint32_t)));
    }
    if (feature_bits) {
        if (!m.fbits.ensure(fw, err)) return text_no_room(fits);
        FR_HIP(hipMemset(m.fbits.p, 0, fw * sizeof(uint32_t)));
    }
    const int grid = (int)std::min<size_t>(n, (size_t)m.grid);
    hipLaunchKernelGGL(text_parse_kernel<2>, dim3(grid), dim3(64), 0, nullptr, (const unsigned char*)m.text.p, (const uint64_t*)m.starts.p, (uint64_t)n,
                       m.recs.p, m.x.p, (uint64_t)d, present_words ? m.pbits.p : (uint32_t*)nullptr, (uint64_t)present_words,
                       feature_bits ? m.fbits.p : (uint32_t*)nullptr);
    FR_HIP(hipGetLastError());
    FR_HIP(hipDeviceSynchronize());
    t->pass2 += text_lap(&clock);
    FR_HIP(hipMemcpy(x, m.x.p, n * d * sizeof(float), hipMemcpyDeviceToHost));
    if (present_words) FR_HIP(hipMemcpy(present_bits, m.pbits.p, n * present_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (feature_bits) FR_HIP(hipMemcpy(feature_bits, m.fbits.p, fw * sizeof(uint32_t), hipMemcpyDeviceToHost));
    t->download += text_lap(&clock);
    return true;
}
