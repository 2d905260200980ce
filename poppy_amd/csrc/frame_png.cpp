// frame_png.cpp — the library's definition of the POPPY_FRAME_PNG hand-off format in plain C++ (include/poppy_hip.h has the rule): a BGR frame as one PNG file
// whose IDAT is a zlib stream of Huffman-only dynamic blocks, a block per POPPY_PNG_SEGMENT_BYTES of the filtered stream, each on one of the eight tables of
// png_tables.h.  kernels_frame_png.hip computes the same bytes on the device; tests/test_host_png.py pins these to a numpy restatement of the rule and to
// zlib's and Pillow's decoders.  The filtered stream and the file's fixed parts are functions of their own (frame_png.h): POPPY_FRAME_PNG_RUNS (frame_png_runs.cpp)
// is the same file around other deflate blocks.  Host only, integer arithmetic only.
#include "frame_png.h"
#include <cstring>

namespace poppy_hip {
namespace png {

namespace {

constexpr Codes kCodes = make_codes();
constexpr CrcTable kCrc = make_crc_table();

void put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

uint32_t crc32_of(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = kCrc.e[(c ^ p[i]) & 255u] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

inline int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// byte j of row y as filter `type` leaves it; the row's bytes are R, G, B of the BGR pixels
inline uint8_t filtered(const uint8_t* row, const uint8_t* above, int j, int type) {
    const int x = j / 3, at = 3 * x + 2 - (j - 3 * x);
    const int cur = row[at], a = x ? row[at - 3] : 0, b = above ? above[at] : 0, c = above && x ? above[at - 3] : 0;
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (uint8_t)(cur - pred);
}

}  // namespace

std::vector<uint8_t> filter_frame(const uint8_t* bgr, size_t stride, int w, int h) {
    const size_t row_bytes = 3 * (size_t)w;
    std::vector<uint8_t> stream((size_t)stream_bytes((size_t)w, (size_t)h));
    for (int y = 0; y < h; ++y) {
        const uint8_t *row = bgr + (size_t)y * stride, *above = y ? row - stride : nullptr;
        int best = 0; unsigned long long best_score = 0;
        for (int type = 0; type < 5; ++type) {
            unsigned long long score = 0;
            for (size_t j = 0; j < row_bytes; ++j) { const int v = filtered(row, above, (int)j, type); score += (unsigned long long)(v < 256 - v ? v : 256 - v); }
            if (type == 0 || score < best_score) { best = type; best_score = score; }
        }
        uint8_t* out = stream.data() + (size_t)y * (1 + row_bytes);
        out[0] = (uint8_t)best;
        for (size_t j = 0; j < row_bytes; ++j) out[1 + j] = filtered(row, above, (int)j, best);
    }
    return stream;
}

void frame_head(uint8_t* dst, int w, int h) {
    memcpy(dst + kOffSignature, kSignature, 8);
    uint8_t* ihdr = dst + kOffIhdr;
    put32(ihdr, 13); memcpy(ihdr + 4, "IHDR", 4); put32(ihdr + 8, (uint32_t)w); put32(ihdr + 12, (uint32_t)h);
    ihdr[16] = 8; ihdr[17] = 2; ihdr[18] = 0; ihdr[19] = 0; ihdr[20] = 0;
    put32(ihdr + 21, crc32_of(ihdr + 4, 17));
    memcpy(dst + kOffIdatType, "IDAT", 4);
    dst[kOffIdatType + 4] = 0x78; dst[kOffIdatType + 5] = 0x01;
}

size_t frame_tail(uint8_t* dst, size_t deflate_bytes, uint32_t adler) {
    const size_t end = kStreamByte + deflate_bytes;         // behind the deflate bytes: Adler-32, the chunk's CRC, IEND
    put32(dst + end, adler);
    put32(dst + kOffIdat, (uint32_t)(end + 4 - (kOffIdatType + 4)));
    put32(dst + end + 4, crc32_of(dst + kOffIdatType, end + 4 - kOffIdatType));
    memcpy(dst + end + 8, kIend, 12);
    const size_t total = end + kTailBytes;
    dst[0] = (uint8_t)total; dst[1] = (uint8_t)(total >> 8); dst[2] = (uint8_t)(total >> 16); dst[3] = (uint8_t)(total >> 24);
    return total;
}

size_t encode_bgr(const uint8_t* bgr, size_t stride, int w, int h, uint8_t* dst) {
    const std::vector<uint8_t> stream = filter_frame(bgr, stride, w, h);
    const size_t n = stream.size();
    frame_head(dst, w, h);
    BitWriter bits{dst + kStreamByte};
    uint32_t adler_a = 1, adler_b = 0;
    for (size_t first = 0; first < n; first += kSegment) {
        const size_t len = n - first < kSegment ? n - first : kSegment;
        const uint8_t* seg = stream.data() + first;
        int table = 0; unsigned long long least = 0;
        for (int k = 0; k < kTables; ++k) {
            unsigned long long cost = (unsigned long long)kHeaderBits[k] + kLen[k][kEob];
            for (size_t i = 0; i < len; ++i) cost += kLen[k][seg[i]];
            if (k == 0 || cost < least) { table = k; least = cost; }
        }
        for (int i = 0; i < kHeaderBits[table]; i += 32) {
            const int nb = kHeaderBits[table] - i < 32 ? kHeaderBits[table] - i : 32;
            bits.put(kHeader[table][i / 32] | (i == 0 && first + len == n ? 1u : 0u), nb);      // BFINAL in the last block
        }
        for (size_t i = 0; i < len; ++i) {
            const uint32_t e = kCodes.e[table][seg[i]];
            bits.put(e >> 4, (int)(e & 15u));
            adler_a = (adler_a + seg[i]) % kAdlerMod; adler_b = (adler_b + adler_a) % kAdlerMod;
        }
        bits.put(kCodes.e[table][kEob] >> 4, (int)(kCodes.e[table][kEob] & 15u));
    }
    bits.pad();
    return frame_tail(dst, bits.at, adler_b << 16 | adler_a);
}

}  // namespace png
}  // namespace poppy_hip

extern "C" {

size_t poppy_png_frame_bytes(const uint8_t* frame) {
    return frame ? (size_t)frame[0] | (size_t)frame[1] << 8 | (size_t)frame[2] << 16 | (size_t)frame[3] << 24 : 0;
}

int poppy_png_table(int k, uint8_t lengths[257], uint8_t* header_bits, int* n_header_bits) {
    using namespace poppy_hip::png;
    if (k < 0 || k >= kTables) return POPPY_E_ARG;
    static_assert(kHeaderWords * 4 <= POPPY_PNG_HEADER_BYTES, "a header fits the caller's buffer");
    if (lengths) memcpy(lengths, kLen[k], kSymbols);
    if (header_bits) {
        memset(header_bits, 0, POPPY_PNG_HEADER_BYTES);
        for (int i = 0; i < kHeaderWords * 4; ++i) header_bits[i] = (uint8_t)(kHeader[k][i / 4] >> (8 * (i & 3)));
    }
    if (n_header_bits) *n_header_bits = kHeaderBits[k];
    return POPPY_OK;
}

int poppy_bgr_to_png_frame(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3) return POPPY_E_ARG;
    if (!png_fits(width, height)) return POPPY_E_UNSUPPORTED;
    poppy_hip::png::encode_bgr(bgr, stride, width, height, dst);
    return POPPY_OK;
}

}  // extern "C"
