// frame_png.h — what the three PNG host statements share (frame_png.cpp defines it; frame_png_runs.cpp and frame_png_opt.cpp use it): the filtered stream, the
// file's fixed parts and the writer of deflate's bits.  POPPY_FRAME_PNG, POPPY_FRAME_PNG_RUNS and POPPY_FRAME_PNG_OPT differ in the deflate blocks only.  Host only.
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
}  // namespace poppy_hip
