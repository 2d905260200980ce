// frame_png.h — what the PNG host statements share (frame_png.cpp defines it; frame_png_runs.cpp, frame_png_opt.cpp and frame_png_seq.cpp use it): the filtered
// stream, the file's fixed parts, the writer of deflate's bits, the token walk of a segment.  POPPY_FRAME_PNG, POPPY_FRAME_PNG_RUNS, POPPY_FRAME_PNG_OPT and
// POPPY_FRAME_PNG_SEQ differ in the deflate blocks only.  Host only.
#pragma once
#include "frame_limits.h"
#include <vector>

namespace poppy_hip {
namespace png {

// the deflate bits, packed from bit 0 of byte 0 up
struct BitWriter {
    uint8_t* p;
    size_t at = 0;
    unsigned long long acc = 0; int n_acc = 0;
    void put(uint32_t value, int n) {                       // n <= 32, value's low n bits
        acc |= (unsigned long long)value << n_acc; n_acc += n;
        while (n_acc >= 8) { p[at++] = (uint8_t)acc; acc >>= 8; n_acc -= 8; }
    }
    void pad() { if (n_acc) put(0, 8 - n_acc); }
};

// the filtered stream of a BGR frame with rows `stride` bytes apart (include/poppy_hip.h: Filtered stream): h * (1 + 3 w) bytes
std::vector<uint8_t> filter_frame(const uint8_t* bgr, size_t stride, int w, int h);
// the signature, IHDR, IDAT's type and the zlib header into dst; the deflate bits begin at dst + kStreamByte
void frame_head(uint8_t* dst, int w, int h);
// behind `deflate_bytes` of deflate data: Adler-32 (given), IDAT's length and CRC, IEND, and `total` into bytes 0..3; returns `total`
size_t frame_tail(uint8_t* dst, size_t deflate_bytes, uint32_t adler);

}  // namespace png

namespace png_runs {

// a segment's tokens in order: f(symbol, extra_bits, extra) — a literal is its byte with no extra bits, a match its length symbol; every match is at distance 1
template <typename F>
void for_each_token(const uint8_t* seg, size_t len, F&& f) {
    for (size_t s = 0; s < len;) {
        size_t e = s + 1;
        while (e < len && seg[e] == seg[s]) ++e;            // the maximal run [s, e): it ends with the segment at the latest
        for (size_t p = s; p < e;) {
            const int t = token_at((int)(e - s), (int)(p - s));      // (never negative: p moves from token to token)
            if (t == 0) { f((int)seg[p], 0, 0u); ++p; }
            else { const Match m = match_of(t); f(m.symbol, m.extra_bits, m.extra); p += (size_t)t; }
        }
        s = e;
    }
}

}  // namespace png_runs

// what POPPY_FRAME_PNG_OPT and POPPY_FRAME_PNG_SEQ share (frame_png_opt.cpp defines it): the canonical codes, the own header of a table, and the coder of a
// filtered stream whose segments have nine candidates — the ninth a table of the segment's own, or one that a whole sequence shares
namespace png_opt {

struct Field { uint32_t value; int bits; };
// deflate's canonical codes by (length, symbol), bit-reversed: entry = reversed code << 4 | length, 0 for a symbol without a code
void canonical_codes(const uint8_t* lengths, int n, uint32_t* entries);
// the own header of a table (include/poppy_hip.h: Block header), BFINAL 0, as fields in order; returns its bits
int own_header(const uint8_t* lengths, std::vector<Field>& out);
// the ninth candidate of every segment of a sequence (POPPY_FRAME_PNG_SEQ): the lengths, their codes and their header
struct SharedTable { uint8_t lengths[kSymbols]; uint32_t code[kSymbols]; std::vector<Field> header; int header_bits; };
// a filtered stream of a w x h frame into dst (POPPY_FRAME_PNG_RUNS' capacity).  shared == null: POPPY_FRAME_PNG_OPT, every segment's ninth candidate is built
// from its own counts; else it is *shared.  Returns `total`.
size_t encode_stream(const std::vector<uint8_t>& stream, int w, int h, const SharedTable* shared, uint8_t* dst);

}  // namespace png_opt
}  // namespace poppy_hip
