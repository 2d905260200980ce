// frame_limits.h — the bounds of a writer's frame that the host statements (frame_resize.cpp, frame_sink.cpp) and the device path (frame_format.cpp, palette_seq.cpp,
// writer_image.cpp) both check, each stated once.  Host only, nothing of HIP.
#pragma once
#include "../../include/poppy_hip.h"
#include "jpeg_tables.h"
#include "png_runs_tables.h"

// poppy_hip_set_frame_size's rule (include/poppy_hip.h): ow x oh is no larger than W x H and at most POPPY_FRAME_SCALE_MAX times smaller per side (so W, H >= 1 too)
inline bool size_admits(int W, int H, int ow, int oh) {
    return ow >= 1 && oh >= 1 && ow <= W && oh <= H && (long long)W <= (long long)POPPY_FRAME_SCALE_MAX * ow && (long long)H <= (long long)POPPY_FRAME_SCALE_MAX * oh;
}
// A coded frame (POPPY_FRAME_GIF, POPPY_FRAME_GIF_SEQ) of w x h pixels.  Its capacity (include/poppy_hip.h has the derivation): `total` and the palette, the
// minimum-code-size byte, every segment's payload at its bound in sub-blocks of 255 bytes behind a length byte each, the terminator ...
inline size_t gif_frame_capacity(size_t w, size_t h) {
    const size_t segments = (w * h + POPPY_GIF_SEGMENT_PIXELS - 1) / POPPY_GIF_SEGMENT_PIXELS, payload = segments * POPPY_GIF_SEGMENT_BYTES;
    return 772 + 1 + payload + (payload + 254) / 255 + 1;
}
constexpr size_t kGifFrameMinBytes = 776;      // ... and the smallest there is, the same with one byte of payload in one sub-block: 772 + 1 + (1 + 1) + 1
inline bool coded_length_ok(size_t total, size_t capacity, size_t least = kGifFrameMinBytes) { return total >= least && total <= capacity; }      // a coder's `total`, before that many bytes are copied or read
// A JPEG-coded frame (POPPY_FRAME_JPEG): `total`, the fixed header, every restart interval at its bound (include/poppy_hip.h has the derivation; jpeg_tables.h) ...
inline size_t jpeg_frame_capacity(size_t w, size_t h, poppy_hip::jpeg::Sampling s = poppy_hip::jpeg::k420) { return (size_t)poppy_hip::jpeg::frame_capacity(w, h, s); }      // (POPPY_FRAME_JPEG444: k444, twice the blocks)
constexpr size_t kJpegFrameMinBytes = poppy_hip::jpeg::kFrameMinBytes;      // ... and the smallest: the header, a byte of entropy-coded data, EOI
// what the format takes: SOF0's 16-bit sides, and a capacity that `total`'s 32 bits hold
inline bool jpeg_fits(int W, int H, poppy_hip::jpeg::Sampling s = poppy_hip::jpeg::k420) { return W <= 65535 && H <= 65535 && poppy_hip::jpeg::frame_capacity((size_t)W, (size_t)H, s) <= 0xffffffffull; }
// the two JPEG formats and the sampling each codes
inline bool format_is_jpeg(int fmt) { return fmt == POPPY_FRAME_JPEG || fmt == POPPY_FRAME_JPEG444; }
inline poppy_hip::jpeg::Sampling format_sampling(int fmt) { return fmt == POPPY_FRAME_JPEG444 ? poppy_hip::jpeg::k444 : poppy_hip::jpeg::k420; }
// A PNG-coded frame (POPPY_FRAME_PNG): `total`, the file's fixed parts and every segment on table 7 at its longest literal (include/poppy_hip.h has the derivation;
// png_tables.h); what the format takes is a capacity below 2^31 bytes, which IDAT's length field and `total` hold; the smallest frame has one byte of deflate data
inline bool png_fits(int W, int H) { return (unsigned long long)W * (unsigned long long)H < (1ull << 31) && poppy_hip::png::frame_capacity((size_t)W, (size_t)H) < (1ull << 31); }
inline size_t png_frame_capacity(size_t w, size_t h) { return (size_t)poppy_hip::png::frame_capacity(w, h); }
constexpr size_t kPngFrameMinBytes = poppy_hip::png::kFrameMinBytes;
// The two PNG formats: POPPY_FRAME_PNG_RUNS is POPPY_FRAME_PNG with runs coded as matches (png_runs_tables.h), the same limits on its own capacity
inline bool format_is_png(int fmt) { return fmt == POPPY_FRAME_PNG || fmt == POPPY_FRAME_PNG_RUNS; }
inline bool png_runs_fits(int W, int H) { return (unsigned long long)W * (unsigned long long)H < (1ull << 31) && poppy_hip::png_runs::frame_capacity((size_t)W, (size_t)H) < (1ull << 31); }
inline size_t png_runs_frame_capacity(size_t w, size_t h) { return (size_t)poppy_hip::png_runs::frame_capacity(w, h); }
inline bool png_fits(int fmt, int W, int H) { return fmt == POPPY_FRAME_PNG_RUNS ? png_runs_fits(W, H) : png_fits(W, H); }
inline size_t png_frame_capacity(int fmt, size_t w, size_t h) { return fmt == POPPY_FRAME_PNG_RUNS ? png_runs_frame_capacity(w, h) : png_frame_capacity(w, h); }
