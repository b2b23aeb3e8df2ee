// Kernels of the device text parser (DESIGN.md, "Text loading"; launched from text_parse.inc).
//   text_count_kernel / text_starts_kernel   a wave takes a slice of TEXT_SCAN_SLICE bytes with 16-byte loads, counts its
//                                            '\n' bytes, and -- once rocPRIM has scanned the counts -- writes the line starts
//   text_parse_kernel<PASS>                  a one-wave workgroup takes a line: stages it into LDS with 16-byte loads, finds
//                                            the token starts with wave ballots, then a lane parses a token (text_number.hpp)
// The text buffer is padded with zero bytes to a whole slice plus one more, so no load here needs a bounds check.
// Nothing is summed: no result depends on lane order.

// 0x80 in every byte of w that equals '\n', exactly (no borrow between bytes)
__device__ __forceinline__ uint32_t tx_newline_bits(uint32_t w) {
    const uint32_t x = w ^ 0x0A0A0A0Au;
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | x | 0x7F7F7F7Fu);
}
__device__ __forceinline__ uint32_t tx_newlines16(const uint4& v) {
    return (uint32_t)(__popc(tx_newline_bits(v.x)) + __popc(tx_newline_bits(v.y)) + __popc(tx_newline_bits(v.z)) + __popc(tx_newline_bits(v.w)));
}

constexpr uint32_t TX_SLICE_VECS = TEXT_SCAN_SLICE / 16;  // 16-byte pieces of a slice
static_assert(TX_SLICE_VECS % 64 == 0, "a wave takes a slice in whole rounds of 64 pieces");

__global__ __launch_bounds__(256) void text_count_kernel(const uint4* __restrict__ text16, uint64_t nslices, uint32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t s = wave; s < nslices; s += nwaves) {
        uint32_t c = 0;
        for (uint32_t j = 0; j < TX_SLICE_VECS; j += 64) c += tx_newlines16(text16[s * TX_SLICE_VECS + j + lane]);
        for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
        if (lane == 0) counts[s] = c;
    }
}

// newline number k of the text (0-based, offsets[s] = newlines before slice s) at byte p ends line k: starts[k + 1] = p + 1
__global__ __launch_bounds__(256) void text_starts_kernel(const uint4* __restrict__ text16, uint64_t nslices, const uint64_t* __restrict__ offsets,
                                                          uint64_t* __restrict__ starts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t s = wave; s < nslices; s += nwaves) {
        uint64_t k = offsets[s];
        for (uint32_t j = 0; j < TX_SLICE_VECS; j += 64) {
            const uint4 v = text16[s * TX_SLICE_VECS + j + lane];
            const uint32_t c = tx_newlines16(v);
            uint32_t incl = c;  // newlines in this round up to and including this lane's piece
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
                if (lane >= (uint32_t)o) incl += up;
            }
            uint64_t at = k + incl - c;
            const uint64_t p0 = (s * TX_SLICE_VECS + j + lane) * 16;
            const uint32_t words[4] = {v.x, v.y, v.z, v.w};
            for (uint32_t w = 0; w < 4; w++) {
                uint32_t bits = tx_newline_bits(words[w]);
                while (bits) {
                    const uint32_t b = (uint32_t)__ffs((int)bits) - 1;  // bit 7 of byte b / 8
                    bits &= bits - 1;
                    starts[++at] = p0 + w * 4 + (b >> 3) + 1;
                }
            }
            k += (uint32_t)__shfl((int)incl, 63);
        }
    }
}

constexpr uint32_t TX_STAGE_VECS = (TEXT_STAGE_LIMIT + 32) / 16;
constexpr uint32_t TX_MAX_TOKENS = TEXT_STAGE_LIMIT / 2 + 1;
static_assert(TEXT_STAGE_LIMIT <= 65535, "token starts are kept as u16");

// PASS 1 writes recs[line]; PASS 2 reads them, parses the unflagged lines again and scatters: x[line * d + fid], the row's
// presence bits (a dense row every index below max_fid + 1, a sparse row the listed ones) and, for sparse rows, fbits.
template <int PASS>
__global__ __launch_bounds__(64) void text_parse_kernel(const unsigned char* __restrict__ text, const uint64_t* __restrict__ starts, uint64_t n,
                                                        frtext::TextLineRec* __restrict__ recs, float* __restrict__ x, uint64_t d,
                                                        uint32_t* __restrict__ pbits, uint64_t pw, uint32_t* __restrict__ fbits) {
    using namespace frtext;
    __shared__ uint4 stage16[TX_STAGE_VECS];
    __shared__ uint16_t tok[TX_MAX_TOKENS];
    const uint32_t lane = threadIdx.x;
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));  // the lanes below this one
    for (uint64_t line = blockIdx.x; line < n; line += gridDim.x) {
        const uint64_t s = starts[line], len64 = starts[line + 1] - 1 - s;
        bool dense = false;
        uint32_t row_max = 0;
        if (PASS == 2) {
            const TextLineRec r = recs[line];
            if (r.reason != R_NONE) continue;
            row_max = r.max_fid;
            dense = (double)r.count / (double)r.max_fid >= 0.5;
        }
        if (len64 > TEXT_STAGE_LIMIT) {  // flagged, never truncated
            if (PASS == 1 && lane == 0) {
                TextLineRec r = {};
                r.reason = R_TOO_LONG;
                recs[line] = r;
            }
            continue;
        }
        const uint32_t L = (uint32_t)len64, a = (uint32_t)(s & 15);
        __syncthreads();  // (the previous line's readers are done with the LDS)
        {
            const uint4* src = reinterpret_cast<const uint4*>(text + (s - a));
            const uint32_t nvec = (a + L + 15) / 16;  // <= TX_STAGE_VECS; ends inside the padded text
            for (uint32_t v = lane; v < nvec; v += 64) stage16[v] = src[v];
        }
        __syncthreads();
        const unsigned char* ln = reinterpret_cast<const unsigned char*>(stage16) + a;
        // ---- token starts of the data part (before the first '#'), in order
        uint32_t ntok = 0, hash = L;
        bool found = false, carry_space = true;
        for (uint32_t c0 = 0; c0 < L && !found; c0 += 64) {
            const uint32_t pos = c0 + lane;
            const unsigned char ch = pos < L ? ln[pos] : (unsigned char)' ';
            const uint64_t hm = __ballot(pos < L && ch == '#');
            const uint64_t spm = __ballot(is_space(ch));
            uint64_t startm = ~spm & ((spm << 1) | (carry_space ? 1ull : 0ull));
            if (hm) {
                const uint32_t hb = (uint32_t)__ffsll((unsigned long long)hm) - 1;
                hash = c0 + hb, found = true;
                startm &= hb == 0 ? 0ull : (~0ull >> (64 - hb));
            }
            if (startm >> lane & 1ull) tok[ntok + (uint32_t)__popcll(startm & below)] = (uint16_t)pos;
            ntok += (uint32_t)__popcll(startm);
            carry_space = (spm >> 63 & 1ull) != 0;
        }
        __syncthreads();
        // ---- the trimmed comment
        uint32_t com0 = hash + 1, com1 = L;
        if (found) {
            while (com0 < com1 && is_space(ln[com0])) com0++;
            while (com1 > com0 && is_space(ln[com1 - 1])) com1--;
        }
        // ---- a token per lane
        uint32_t key = 255;  // the smallest reason met (255: none)
        uint32_t maxfid = 0, qoff = 0, qlen = 0;
        float label = 0.0f;
        int carry_fid = -1;
        if (ntok < 3) key = R_GRAMMAR;
        for (uint32_t b = 0; b < ntok; b += 64) {
            const uint32_t t = b + lane;
            int fid = -1;
            uint32_t r = R_NONE;
            if (t < ntok) {
                const uint32_t st = tok[t];
                uint32_t e = st;
                while (e < hash && !is_space(ln[e])) e++;
                const unsigned char* p = ln + st;
                const uint32_t len = e - st;
                double v = 0.0;
                if (t == 0) {
                    r = fast_number(p, len, &v);
                    label = (float)v;
                } else if (t == 1) {
                    const bool q0 = len > 4 && p[0] == 'q' && p[1] == 'i' && p[2] == 'd' && p[3] == ':';
                    const bool q1 = len >= 8 && p[4] == 'q' && p[5] == 'i' && p[6] == 'd' && p[7] == ':';
                    if (!q0 || q1) r = R_GRAMMAR;
                    qoff = st + 4, qlen = len - 4;
                } else {
                    uint32_t c = 0, f = 0;
                    while (c < len && p[c] != ':') c++;
                    if (c == len || !fast_fid(p, c, &f)) {
                        r = R_GRAMMAR;
                    } else {
                        fid = (int)f;
                        maxfid = maxfid > f ? maxfid : f;
                        r = fast_number(p + c + 1, len - c - 1, &v);
                        if (PASS == 2 && r == R_NONE) {
                            x[line * d + f] = (float)v;
                            if (!dense) {
                                if (pbits) atomicOr(&pbits[line * pw + (f >> 5)], 1u << (f & 31));
                                if (fbits) atomicOr(&fbits[f >> 5], 1u << (f & 31));
                            }
                        }
                    }
                }
            }
            int prev = __shfl_up(fid, 1);
            if (lane == 0) prev = carry_fid;
            carry_fid = __shfl(fid, 63);
            if (t < ntok && t >= 2 && fid >= 0 && fid <= prev && (r == R_NONE || r > R_UNSORTED)) r = R_UNSORTED;
            if (r != R_NONE && r < key) key = r;
            if (b == 0) {
                label = __shfl(label, 0);
                qoff = (uint32_t)__shfl((int)qoff, 1), qlen = (uint32_t)__shfl((int)qlen, 1);
            }
        }
        if (PASS == 1) {
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t ok = (uint32_t)__shfl_xor((int)key, o), om = (uint32_t)__shfl_xor((int)maxfid, o);
                key = ok < key ? ok : key;
                maxfid = om > maxfid ? om : maxfid;
            }
            if (lane == 0) {
                TextLineRec r = {};
                r.reason = key == 255 ? (uint32_t)R_NONE : key;
                if (r.reason == R_NONE) {
                    r.label = label;
                    r.qid_off = qoff, r.qid_len = qlen;
                    r.com_off = found ? com0 : 0, r.com_len = found ? com1 - com0 : 0;
                    r.has_hash = found ? 1u : 0u;
                    r.count = ntok - 2, r.max_fid = maxfid;
                }
                recs[line] = r;
            }
        } else if (dense && pbits) {
            const uint32_t last = row_max >> 5;
            for (uint32_t w = lane; w <= last; w += 64)
                pbits[line * pw + w] = (w < last || (row_max & 31) == 31) ? 0xFFFFFFFFu : ((1u << ((row_max & 31) + 1)) - 1u);
        }
    }
}
