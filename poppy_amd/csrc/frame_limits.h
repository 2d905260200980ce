// frame_limits.h — what a writer's frame format is, stated once: one record per POPPY_FRAME_* format (kFormats, format_traits) and the bounds of a frame that the
// host statements (frame_resize.cpp, frame_sink.cpp) and the device path (frame_format.cpp, palette_seq.cpp, writer_image.cpp) both check.  Host only, nothing of HIP.
#pragma once
#include "../../include/poppy_hip.h"
#include "jpeg_tables.h"
#include "png_opt.h"

// poppy_hip_set_frame_size's rule (include/poppy_hip.h): ow x oh is no larger than W x H and at most POPPY_FRAME_SCALE_MAX times smaller per side (so W, H >= 1 too)
inline bool size_admits(int W, int H, int ow, int oh) {
    return ow >= 1 && oh >= 1 && ow <= W && oh <= H && (long long)W <= (long long)POPPY_FRAME_SCALE_MAX * ow && (long long)H <= (long long)POPPY_FRAME_SCALE_MAX * oh;
}
// A GIF-coded frame of w x h pixels.  Its capacity (include/poppy_hip.h has the derivation): `total` and the palette, the minimum-code-size byte, every segment's
// payload at its bound in sub-blocks of 255 bytes behind a length byte each, the terminator ...
inline size_t gif_frame_capacity(size_t w, size_t h) {
    const size_t segments = (w * h + POPPY_GIF_SEGMENT_PIXELS - 1) / POPPY_GIF_SEGMENT_PIXELS, payload = segments * POPPY_GIF_SEGMENT_BYTES;
    return 772 + 1 + payload + (payload + 254) / 255 + 1;
}
constexpr size_t kGifFrameMinBytes = 776;      // ... and the smallest there is, the same with one byte of payload in one sub-block: 772 + 1 + (1 + 1) + 1
inline bool coded_length_ok(size_t total, size_t capacity, size_t least) { return total >= least && total <= capacity; }      // a coder's `total` between its record's `least` and the capacity, before that many bytes are copied or read
// A JPEG-coded frame: what the format takes is SOF0's 16-bit sides, and a capacity (jpeg_tables.h; include/poppy_hip.h has the derivation) that `total`'s 32 bits hold
inline bool jpeg_fits(int W, int H, poppy_hip::jpeg::Sampling s = poppy_hip::jpeg::k420) { return W <= 65535 && H <= 65535 && poppy_hip::jpeg::frame_capacity((size_t)W, (size_t)H, s) <= 0xffffffffull; }
// ... and the same on per-frame tables (POPPY_FRAME_JPEG_OPT, POPPY_FRAME_JPEG444_OPT), on their own capacity
inline bool jpeg_opt_fits(int W, int H, poppy_hip::jpeg::Sampling s = poppy_hip::jpeg::k420) { return W <= 65535 && H <= 65535 && poppy_hip::jpeg::opt_frame_capacity((size_t)W, (size_t)H, s) <= 0xffffffffull; }
// ... and a sequence of n such frames on one table set (POPPY_FRAME_JPEG_SEQ, POPPY_FRAME_JPEG444_SEQ): with B the blocks of a frame over all components, n * B * 64
// symbols at the most, so that every summed table stays below the table rule's refusal and the device adds and merges in 32 bits (include/poppy_hip.h: Limits)
inline bool jpeg_seq_fits(int n, int W, int H, poppy_hip::jpeg::Sampling s = poppy_hip::jpeg::k420) {
    if (n < 1 || !jpeg_opt_fits(W, H, s)) return false;
    const unsigned long long per_frame = (unsigned long long)poppy_hip::jpeg::mcu_count((size_t)W, (size_t)H, s) * poppy_hip::jpeg::mcu_blocks(s) * 64ull;      // (< 2^30: the count bound)
    return (unsigned long long)n <= POPPY_JPEG_SEQ_MAX_SYMBOLS / per_frame;
}
// A PNG-coded frame: what the format takes is a capacity (png_tables.h; with runs coded as matches png_runs_tables.h) below 2^31 bytes, which IDAT's length field and `total` hold
inline bool png_fits(int W, int H) { return (unsigned long long)W * (unsigned long long)H < (1ull << 31) && poppy_hip::png::frame_capacity((size_t)W, (size_t)H) < (1ull << 31); }
inline bool png_runs_fits(int W, int H) { return (unsigned long long)W * (unsigned long long)H < (1ull << 31) && poppy_hip::png_runs::frame_capacity((size_t)W, (size_t)H) < (1ull << 31); }
// ... and a sequence of n such frames on one table (POPPY_FRAME_PNG_SEQ): a segment of s bytes has at most s tokens and one end-of-block, so with n_bytes the stream's
// bytes and S its segments, n * (n_bytes + S) bounds the sum of the sequence's counts; at most POPPY_PNG_SEQ_MAX_SYMBOLS keeps it below the length rule's refusal
// and lets the device add in 32 bits (include/poppy_hip.h: Limits)
constexpr bool png_seq_symbols_fit(unsigned long long n, unsigned long long w, unsigned long long h) {
    const unsigned long long n_bytes = h * (1 + 3 * w), segments = (n_bytes + POPPY_PNG_SEGMENT_BYTES - 1) / POPPY_PNG_SEGMENT_BYTES;
    return n >= 1 && n <= POPPY_PNG_SEQ_MAX_SYMBOLS / (n_bytes + segments);
}
static_assert(png_seq_symbols_fit(858993459, 1, 1) && !png_seq_symbols_fit(858993460, 1, 1), "1 x 1: 4 bytes and a segment, 5 * 858993459 = 2^32 - 1 is the last sequence admitted");
static_assert(png_seq_symbols_fit((1u << 29) - 1, 2, 1) && !png_seq_symbols_fit(1u << 29, 2, 1), "2 x 1: 7 bytes and a segment, 8 * 2^29 = 2^32 is refused");
static_assert(png_seq_symbols_fit(690, 1920, 1080) && !png_seq_symbols_fit(691, 1920, 1080), "include/poppy_hip.h states 690 frames at 1080p");
inline bool png_seq_fits(int n, int W, int H) { return n >= 1 && W >= 1 && H >= 1 && png_runs_fits(W, H) && png_seq_symbols_fit((unsigned long long)n, (unsigned long long)W, (unsigned long long)H); }

// The record of a format.  A frame reaches its writer in up to two steps behind the BGR frame: the raster step (the BGR frame as planes or as palette indices) and
// the coder step, which reads the raster form (PNG: the BGR frame itself) and gives a frame whose length its own bytes decide.
enum FrameRaster { kRasterNone = 0, kRasterI420, kRasterI444, kRasterPal8 };      // none: the BGR frame itself
enum FrameCoder { kCoderNone = 0, kCoderGif, kCoderJpeg, kCoderPng };
struct FormatTraits {
    int format;                // the POPPY_FRAME_* constant
    const char* name;          // for messages: a coded format's is its coder's ("JPEG frame coding: ")
    FrameRaster raster;
    FrameCoder coder;
    int variant;               // the JPEG coder's sampling (jpeg::Sampling); the PNG coder's tokens and tables (png::Variant): literals, runs as matches, those on the segments' own tables, or on the sequence's one table
    bool frame_tables;         // the JPEG coder's Huffman tables: the Annex K examples (false), or four tables built from symbol counts — this frame's own, or (sequence) the sequence's sums
    bool sequence;             // one palette (PAL8), one Huffman table set (JPEG) or one ninth table (PNG) for all the frames a call hands to its writer: they wait in the sequence store until the last
                               // is rendered (palette_seq.h), and no slot converts or codes them — the sequence pass and the sequence's coder do
    size_t least;              // the smallest `total` its coder gives (coded_length_ok's lower bound)
    // a frame whose length its bytes decide: poppy_frame_bytes is its capacity, the writer is told stride 0, a pinned word holds its length
    constexpr bool coded() const { return coder != kCoderNone; }
    // what a slot's own conversion does (enqueue_conversion) and has buffers for: nothing under a sequence format
    constexpr FrameRaster slot_raster() const { return sequence ? kRasterNone : raster; }
    constexpr FrameCoder slot_coder() const { return sequence ? kCoderNone : coder; }
    constexpr bool converts() const { return slot_raster() != kRasterNone || slot_coder() != kCoderNone; }
    constexpr poppy_hip::jpeg::Sampling sampling() const { return variant ? poppy_hip::jpeg::k444 : poppy_hip::jpeg::k420; }
    constexpr bool runs() const { return variant != poppy_hip::png::kLiterals; }      // PNG: runs coded as matches, on POPPY_FRAME_PNG_RUNS' capacity
};
inline constexpr FormatTraits kFormats[] = {
    {POPPY_FRAME_BGR,         "BGR",  kRasterNone, kCoderNone, 0,                     false, false, 0},
    {POPPY_FRAME_I420,        "I420", kRasterI420, kCoderNone, 0,                     false, false, 0},
    {POPPY_FRAME_PAL8,        "PAL8", kRasterPal8, kCoderNone, 0,                     false, false, 0},
    {POPPY_FRAME_PAL8_SEQ,    "PAL8", kRasterPal8, kCoderNone, 0,                     false, true,  0},
    {POPPY_FRAME_GIF,         "GIF",  kRasterPal8, kCoderGif,  0,                     false, false, kGifFrameMinBytes},
    {POPPY_FRAME_GIF_SEQ,     "GIF",  kRasterPal8, kCoderGif,  0,                     false, true,  kGifFrameMinBytes},
    {POPPY_FRAME_JPEG,        "JPEG", kRasterI420, kCoderJpeg, poppy_hip::jpeg::k420, false, false, poppy_hip::jpeg::kFrameMinBytes},      // the header, a byte of entropy-coded data, EOI
    {POPPY_FRAME_JPEG444,     "JPEG", kRasterI444, kCoderJpeg, poppy_hip::jpeg::k444, false, false, poppy_hip::jpeg::kFrameMinBytes},      // (twice the blocks)
    {POPPY_FRAME_JPEG_OPT,    "JPEG", kRasterI420, kCoderJpeg, poppy_hip::jpeg::k420, true,  false, poppy_hip::jpeg::kOptFrameMinBytes},   // the header with four one-symbol tables, a byte of data, EOI
    {POPPY_FRAME_JPEG444_OPT, "JPEG", kRasterI444, kCoderJpeg, poppy_hip::jpeg::k444, true,  false, poppy_hip::jpeg::kOptFrameMinBytes},
    {POPPY_FRAME_JPEG_SEQ,    "JPEG", kRasterI420, kCoderJpeg, poppy_hip::jpeg::k420, true,  true,  poppy_hip::jpeg::kOptFrameMinBytes},   // JPEG_OPT's frames on one table set per sequence
    {POPPY_FRAME_JPEG444_SEQ, "JPEG", kRasterI444, kCoderJpeg, poppy_hip::jpeg::k444, true,  true,  poppy_hip::jpeg::kOptFrameMinBytes},
    {POPPY_FRAME_PNG,         "PNG",  kRasterNone, kCoderPng,  0,                     false, false, poppy_hip::png::kFrameMinBytes},       // the file's fixed parts and one byte of deflate data
    {POPPY_FRAME_PNG_RUNS,    "PNG",  kRasterNone, kCoderPng,  poppy_hip::png::kRuns, false, false, poppy_hip::png::kFrameMinBytes},       // PNG with runs coded as matches, the same limits on its own capacity
    {POPPY_FRAME_PNG_OPT,     "PNG",  kRasterNone, kCoderPng,  poppy_hip::png::kRunsOwn, false, false, poppy_hip::png::kFrameMinBytes},    // PNG_RUNS with a ninth table per segment, built from its counts: PNG_RUNS' limits and capacity
    {POPPY_FRAME_PNG_SEQ,     "PNG",  kRasterNone, kCoderPng,  poppy_hip::png::kRunsSeq, false, true,  poppy_hip::png::kFrameMinBytes},    // PNG_OPT's frames on one ninth table per sequence, built from the sequence's summed counts
};
constexpr const FormatTraits* format_traits(int fmt) {      // null for an unknown format
    for (const FormatTraits& t : kFormats) if (t.format == fmt) return &t;
    return nullptr;
}

// what the writer is told: 0 for a coded frame, the width for the planar and palette formats, 3 * width for BGR
constexpr size_t format_stride(const FormatTraits& t, int W) { return t.coded() ? 0 : t.raster == kRasterNone ? (size_t)W * 3 : (size_t)W; }
// the bytes of a w x h frame in a raster form (none: the tight BGR frame)
constexpr size_t raster_bytes(FrameRaster r, size_t w, size_t h) {
    return r == kRasterI420 ? w * h + 2 * ((w + 1) / 2) * ((h + 1) / 2) : r == kRasterPal8 ? w * h + 768 : w * h * 3;
}
// what the format's coder takes (a format without one: every frame; the palette's own limit is format_refuses')
inline bool fits(const FormatTraits& t, int W, int H) {
    return t.coder == kCoderJpeg ? (t.frame_tables ? jpeg_opt_fits(W, H, t.sampling()) : jpeg_fits(W, H, t.sampling())) : t.coder == kCoderPng ? (t.runs() ? png_runs_fits(W, H) : png_fits(W, H)) : t.coder == kCoderGif ? W <= 65535 && H <= 65535 : true;
}
// a coded frame's capacity, an upper bound of `total` for any content (include/poppy_hip.h has the derivations)
inline size_t capacity(const FormatTraits& t, size_t w, size_t h) {
    return t.coder == kCoderJpeg ? (size_t)(t.frame_tables ? poppy_hip::jpeg::opt_frame_capacity(w, h, t.sampling()) : poppy_hip::jpeg::frame_capacity(w, h, t.sampling())) :
           t.coder == kCoderPng ? (size_t)(t.runs() ? poppy_hip::png_runs::frame_capacity(w, h) : poppy_hip::png::frame_capacity(w, h)) : t.coder == kCoderGif ? gif_frame_capacity(w, h) : 0;
}
// poppy_frame_bytes of a frame with positive sides: the raster form's bytes, or the capacity (PNG: nothing to size where the format refuses)
inline size_t frame_bytes(const FormatTraits& t, int W, int H) {
    if (!t.coded()) return raster_bytes(t.raster, (size_t)W, (size_t)H);
    return t.coder == kCoderPng && !fits(t, W, H) ? 0 : capacity(t, (size_t)W, (size_t)H);
}

// every constant of include/poppy_hip.h has exactly one record, and the records hold what the code relies on
constexpr bool formats_hold() {
    constexpr int all[] = {POPPY_FRAME_BGR, POPPY_FRAME_I420, POPPY_FRAME_PAL8, POPPY_FRAME_PAL8_SEQ, POPPY_FRAME_GIF, POPPY_FRAME_GIF_SEQ, POPPY_FRAME_JPEG, POPPY_FRAME_JPEG444,
                           POPPY_FRAME_PNG, POPPY_FRAME_PNG_RUNS, POPPY_FRAME_JPEG_OPT, POPPY_FRAME_JPEG444_OPT, POPPY_FRAME_PNG_OPT, POPPY_FRAME_JPEG_SEQ, POPPY_FRAME_JPEG444_SEQ,
                           POPPY_FRAME_PNG_SEQ};
    if (sizeof all / sizeof *all != sizeof kFormats / sizeof *kFormats) return false;
    for (int fmt : all) {
        int n = 0;
        for (const FormatTraits& t : kFormats) n += t.format == fmt;
        if (n != 1) return false;
    }
    for (const FormatTraits& t : kFormats) {
        if (t.sequence && (t.slot_coder() != kCoderNone || t.slot_raster() != kRasterNone)) return false;      // a sequence format has no per-slot coder (and no raster step)
        const bool palette_seq = t.raster == kRasterPal8 && (t.coder == kCoderNone || t.coder == kCoderGif), table_seq = t.coder == kCoderJpeg && t.frame_tables;
        const bool png_seq = t.coder == kCoderPng && t.variant == poppy_hip::png::kRunsSeq;
        if (t.sequence && !palette_seq && !table_seq && !png_seq) return false;      // ... and is PAL8 under one palette, bare or GIF-coded, JPEG under one table set, or PNG under one ninth table (palette_seq.cpp)
        if (png_seq && !t.sequence) return false;                       // ... which only a sequence has
        if ((format_stride(t, 1) == 0) != t.coded()) return false;      // only a coded format reports stride 0
        if (t.coded() != (t.least > 0)) return false;                   // ... and it alone has a smallest `total`
        if (t.coder == kCoderGif && t.raster != kRasterPal8) return false;      // the coders read their raster form: GIF PAL8, JPEG the planes of its sampling, PNG the BGR frame
        if (t.coder == kCoderJpeg && t.raster != (t.sampling() == poppy_hip::jpeg::k444 ? kRasterI444 : kRasterI420)) return false;
        if (t.coder == kCoderPng && t.raster != kRasterNone) return false;
        if (t.coder == kCoderPng && t.variant != poppy_hip::png::kLiterals && t.variant != poppy_hip::png::kRuns && t.variant != poppy_hip::png::kRunsOwn && t.variant != poppy_hip::png::kRunsSeq) return false;
        if (t.coder == kCoderPng && t.least != poppy_hip::png::kFrameMinBytes) return false;      // every PNG variant's smallest frame is the fixed parts and a byte of data
        if (t.frame_tables && t.coder != kCoderJpeg) return false;      // per-frame tables are the JPEG coder's, and such a format's smallest frame is the OPT header's
        if (t.coder == kCoderJpeg && t.least != (t.frame_tables ? poppy_hip::jpeg::kOptFrameMinBytes : poppy_hip::jpeg::kFrameMinBytes)) return false;
    }
    return true;
}
static_assert(formats_hold(), "kFormats: one record per POPPY_FRAME_* constant; a sequence format has no per-slot coder; only a coded format reports stride 0");
