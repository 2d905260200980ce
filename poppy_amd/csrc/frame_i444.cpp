// frame_i444.cpp — the library's definition of the I444 planes that POPPY_FRAME_JPEG444 codes (include/poppy_hip.h has the rule): three tight width x height
// planes, Y then U then V, full-range BT.601 with 16 fractional bits, per pixel.  Y is poppy_bgr_to_i420's Y, U and V are its formulas on one pixel, and all three
// are what POPPY_SINK_Y4M writes (frame_sink.cpp).  kernels_frame_i444.hip computes the same bytes on the device.  Host only, integer arithmetic only.
#include "../../include/poppy_hip.h"

extern "C" {

int poppy_bgr_to_i444(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3) return POPPY_E_ARG;
    auto clamp = [](int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); };
    const size_t plane = (size_t)width * height;
    for (int y = 0; y < height; ++y) {
        const uint8_t* p = bgr + (size_t)y * stride;
        uint8_t* o = dst + (size_t)y * width;
        for (int x = 0; x < width; ++x) {
            const int b = p[3 * x], g = p[3 * x + 1], r = p[3 * x + 2];
            o[x] = clamp((19595 * r + 38470 * g + 7471 * b + 32768) >> 16);
            o[plane + x] = clamp(((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128);      // (>> of a negative int: arithmetic)
            o[2 * plane + x] = clamp(((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128);
        }
    }
    return POPPY_OK;
}

}  // extern "C"
