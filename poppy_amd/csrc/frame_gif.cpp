// frame_gif.cpp — the library's definition of the POPPY_FRAME_GIF and POPPY_FRAME_GIF_SEQ hand-off formats in plain C++ (include/poppy_hip.h): a PAL8 frame whose index plane is LZW-coded in
// independent segments of POPPY_GIF_SEGMENT_PIXELS pixels and framed as GIF image data.  The coder is the GIF sinks' (gif_lzw.h); kernels_frame_gif.hip computes the
// same bytes on the device, tests/test_host_gif_coded.py pins these to a plain-Python restatement of the rule.
#include "../../include/poppy_hip.h"
#include "gif_lzw.h"
#include <cstring>
#include <vector>

namespace {

constexpr size_t kGifHead = 772;                            // `total` and the palette

bool gif_fits(int width, int height) {
    return width <= 65535 && height <= 65535 && (unsigned long long)width * (unsigned long long)height <= (unsigned long long)POPPY_PAL8_MAX_PIXELS;
}

// the packed bytes behind the minimum-code-size byte, in sub-blocks of 255 (framed on the fly: a length byte in front of every 255, filled in when its block is known)
struct SubBlocks {
    uint8_t* dst;                                           // the byte behind the minimum code size
    size_t n = 0;                                           // payload bytes so far
    void operator()(uint8_t byte) { dst[n + n / 255 + 1] = byte; ++n; }
    // length bytes and the terminator; returns the bytes used from dst on
    size_t close() {
        for (size_t b = 0; b * 255 < n; ++b) dst[b * 256] = (uint8_t)(n - b * 255 >= 255 ? 255 : n - b * 255);
        const size_t end = n + (n + 254) / 255;
        dst[end] = 0;
        return end + 1;
    }
};

}  // namespace

extern "C" {

size_t poppy_gif_frame_bytes(const uint8_t* frame) {
    return frame ? (size_t)frame[0] | (size_t)frame[1] << 8 | (size_t)frame[2] << 16 | (size_t)frame[3] << 24 : 0;
}

int poppy_pal8_to_gif_frame(const uint8_t* pal8, int width, int height, uint8_t* dst) {
    if (!pal8 || !dst || width <= 0 || height <= 0) return POPPY_E_ARG;
    if (!gif_fits(width, height)) return POPPY_E_UNSUPPORTED;
    using poppy_hip::GifLzwCoder;
    const size_t n = (size_t)width * height, S = POPPY_GIF_SEGMENT_PIXELS;
    memcpy(dst + 4, pal8 + n, 768);
    dst[kGifHead] = 8;                                      // the minimum code size
    SubBlocks out{dst + kGifHead + 1};
    GifLzwCoder z;
    for (size_t at = 0; at < n; at += S) {
        const size_t len = n - at < S ? n - at : S;
        const int w = z.run(pal8 + at, len, out);
        if (at + len < n) {                                 // a clear code at the current width, then 9-bit clear codes up to a byte boundary (9 = 1 mod 8: seven at most)
            z.put(GifLzwCoder::kClear, w, out);
            while (z.n_acc) z.put(GifLzwCoder::kClear, 9, out);
        } else {
            z.put(GifLzwCoder::kEnd, w, out);
            z.flush(out);
        }
    }
    const size_t total = kGifHead + 1 + out.close();
    dst[0] = (uint8_t)total; dst[1] = (uint8_t)(total >> 8); dst[2] = (uint8_t)(total >> 16); dst[3] = (uint8_t)(total >> 24);
    return POPPY_OK;
}

int poppy_bgr_to_gif_frame(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3) return POPPY_E_ARG;
    if (!gif_fits(width, height)) return POPPY_E_UNSUPPORTED;
    std::vector<uint8_t> pal8(poppy_frame_bytes(POPPY_FRAME_PAL8, width, height));
    const int rc = poppy_bgr_to_pal8(bgr, stride, width, height, pal8.data());
    return rc ? rc : poppy_pal8_to_gif_frame(pal8.data(), width, height, dst);
}

// POPPY_FRAME_GIF_SEQ: the composition of the two statements — the sequence's PAL8_SEQ frames, each coded.  The limits are checked here, on the arguments alone,
// so that nothing is read or written when either statement would refuse.
int poppy_bgr_frames_to_gif_frames(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3 || n_frames < 1) return POPPY_E_ARG;
    if (!gif_fits(width, height)) return POPPY_E_UNSUPPORTED;
    if ((unsigned long long)n_frames * (unsigned long long)width * (unsigned long long)height >= POPPY_PAL8_SEQ_MAX_PIXELS) return POPPY_E_UNSUPPORTED;
    const size_t pal8_bytes = poppy_frame_bytes(POPPY_FRAME_PAL8_SEQ, width, height), capacity = poppy_frame_bytes(POPPY_FRAME_GIF_SEQ, width, height);
    std::vector<uint8_t> pal8(pal8_bytes * (size_t)n_frames);
    int rc = poppy_bgr_frames_to_pal8(bgr, stride, frame_stride, n_frames, width, height, pal8.data());
    for (int k = 0; k < n_frames && rc == POPPY_OK; ++k) rc = poppy_pal8_to_gif_frame(pal8.data() + (size_t)k * pal8_bytes, width, height, dst + (size_t)k * capacity);
    return rc;
}

}  // extern "C"
