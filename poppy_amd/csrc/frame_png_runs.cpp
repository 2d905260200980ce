// frame_png_runs.cpp — the library's definition of the POPPY_FRAME_PNG_RUNS hand-off format in plain C++ (include/poppy_hip.h has the rule): POPPY_FRAME_PNG's
// file (frame_png.cpp: the filtered stream, the fixed parts), with every segment's runs of equal bytes coded as deflate matches at distance 1 on one of the eight
// tables of png_runs_tables.h.  kernels_frame_png.hip computes the same bytes on the device; tests/test_host_png_runs.py pins these to a numpy restatement of
// the rule and to zlib's and Pillow's decoders.  Host only, integer arithmetic only.
#include "frame_png.h"
#include <cstring>

namespace poppy_hip {
namespace png_runs {

namespace {

constexpr Codes kCodes = make_codes();

}  // namespace

size_t encode_bgr(const uint8_t* bgr, size_t stride, int w, int h, uint8_t* dst) {
    using png::kAdlerMod;
    const std::vector<uint8_t> stream = png::filter_frame(bgr, stride, w, h);
    const size_t n = stream.size();
    png::frame_head(dst, w, h);
    png::BitWriter bits{dst + kStreamByte};
    uint32_t adler_a = 1, adler_b = 0;
    for (size_t first = 0; first < n; first += kSegment) {
        const size_t len = n - first < kSegment ? n - first : kSegment;
        const uint8_t* seg = stream.data() + first;
        unsigned long long cost[kTables];
        for (int k = 0; k < kTables; ++k) cost[k] = (unsigned long long)kHeaderBits[k] + kLen[k][kEob];
        for_each_token(seg, len, [&](int symbol, int extra_bits, uint32_t) {
            for (int k = 0; k < kTables; ++k) cost[k] += (unsigned long long)kLen[k][symbol] + (symbol > kEob ? extra_bits + 1 : 0);      // (a match: its extra bits and the distance code's bit)
        });
        int table = 0;
        for (int k = 1; k < kTables; ++k) if (cost[k] < cost[table]) table = k;
        for (int i = 0; i < kHeaderBits[table]; i += 32) {
            const int nb = kHeaderBits[table] - i < 32 ? kHeaderBits[table] - i : 32;
            bits.put(kHeader[table][i / 32] | (i == 0 && first + len == n ? 1u : 0u), nb);      // BFINAL in the last block
        }
        for_each_token(seg, len, [&](int symbol, int extra_bits, uint32_t extra) {
            const uint32_t e = kCodes.e[table][symbol];
            bits.put(e >> 4, (int)(e & 15u));
            if (symbol > kEob) bits.put(extra, extra_bits + 1);      // the extra bits, then distance symbol 0: the one code of its table, a 0 bit
        });
        bits.put(kCodes.e[table][kEob] >> 4, (int)(kCodes.e[table][kEob] & 15u));
        for (size_t i = 0; i < len; ++i) { adler_a = (adler_a + seg[i]) % kAdlerMod; adler_b = (adler_b + adler_a) % kAdlerMod; }
    }
    bits.pad();
    return png::frame_tail(dst, bits.at, adler_b << 16 | adler_a);
}

}  // namespace png_runs
}  // namespace poppy_hip

extern "C" {

int poppy_png_runs_table(int k, uint8_t lengths[286], uint8_t* header_bits, int* n_header_bits) {
    using namespace poppy_hip::png_runs;
    if (k < 0 || k >= kTables) return POPPY_E_ARG;
    if (lengths) memcpy(lengths, kLen[k], kSymbols);
    if (header_bits) {
        memset(header_bits, 0, POPPY_PNG_HEADER_BYTES);
        for (int i = 0; i < kHeaderWords * 4; ++i) header_bits[i] = (uint8_t)(kHeader[k][i / 4] >> (8 * (i & 3)));
    }
    if (n_header_bits) *n_header_bits = kHeaderBits[k];
    return POPPY_OK;
}

int poppy_bgr_to_png_runs_frame(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3) return POPPY_E_ARG;
    if (!png_runs_fits(width, height)) return POPPY_E_UNSUPPORTED;
    poppy_hip::png_runs::encode_bgr(bgr, stride, width, height, dst);
    return POPPY_OK;
}

}  // extern "C"
