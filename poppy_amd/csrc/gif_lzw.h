// gif_lzw.h — the library's one LZW coder (host side), shared by the GIF sinks (frame_sink.cpp: one stream per image, closed by an end code) and by the
// POPPY_FRAME_GIF hand-off format (frame_gif.cpp: segments that each begin with a clear code).  kernels_frame_gif.hip codes the same bytes on the device.
//
// GIF's variable-width LZW (minimum code size 8): codes 0..255 the bytes, 256 clear, 257 end, strings from 258; the width grows from 9 to 12 bits
// when the entry just added is the first that needs the next width (what decoders mirror one entry behind), and a clear code restarts the table
// when it is full.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace poppy_hip {

struct GifLzwCoder {
    static constexpr int kClear = 256, kEnd = 257;
    static constexpr int kHash = 8192;                      // open addressing over (prefix << 8 | byte); at most 3838 strings live
    uint32_t acc = 0; int n_acc = 0;                        // the bits not yet handed on as whole bytes
    std::vector<uint32_t> key; std::vector<uint16_t> val;
    GifLzwCoder() : key(kHash), val(kHash) {}
    // `out(byte)` takes the packed bytes in order
    template <class Out> void put(int code, int width, Out& out) {
        acc |= (uint32_t)code << n_acc; n_acc += width;
        while (n_acc >= 8) { out((uint8_t)acc); acc >>= 8; n_acc -= 8; }
    }
    // the last bits, padded with zeros to a byte
    template <class Out> void flush(Out& out) { if (n_acc) { out((uint8_t)acc); acc = 0; n_acc = 0; } }
    void reset() { std::fill(key.begin(), key.end(), 0xffffffffu); }
    // A clear code at 9 bits, then the codes of px[0 .. n), n >= 1, the last string's code included.  Returns the width the NEXT code has to be written with (an
    // end code or a clear code: the caller's).
    template <class Out> int run(const uint8_t* px, size_t n, Out& out) {
        int width = 9, next = 258;
        reset();
        put(kClear, width, out);
        int prefix = px[0];
        for (size_t i = 1; i < n; ++i) {
            const uint32_t k = ((uint32_t)prefix << 8) | px[i];
            uint32_t h = (k * 2654435761u) >> 19;            // 13 bits
            while (key[h] != 0xffffffffu && key[h] != k) h = (h + 1) & (kHash - 1);
            if (key[h] == k) { prefix = val[h]; continue; }
            put(prefix, width, out);
            if (next == 4096) { put(kClear, width, out); reset(); width = 9; next = 258; }
            else { key[h] = k; val[h] = (uint16_t)next; if (next == (1 << width)) ++width; ++next; }
            prefix = px[i];
        }
        put(prefix, width, out);
        return width;
    }
};

}  // namespace poppy_hip
