// frame_scale.cpp — the host side of the scaled hand-off (include/poppy_hip.h: poppy_hip_set_frame_scale): the scaled size of a frame and poppy_bgr_downscale,
// the library's definition of a frame scaled down by a whole factor (kernels_frame_scale.hip computes the same bytes on the device).
#include "../../include/poppy_hip.h"

extern "C" {

int poppy_frame_scaled_size(int width, int height, int factor, int* ow, int* oh) {
    if (width <= 0 || height <= 0 || factor < 1 || factor > POPPY_FRAME_SCALE_MAX || !ow || !oh) return POPPY_E_ARG;
    *ow = (int)(((long long)width + factor - 1) / factor);
    *oh = (int)(((long long)height + factor - 1) / factor);
    return POPPY_OK;
}

// output pixel (x, y): per channel (sum + n / 2) / n over source columns [s x, min(s x + s, width)) and rows [s y, min(s y + s, height)), n pixels
int poppy_bgr_downscale(const uint8_t* bgr, size_t stride, int width, int height, int factor, uint8_t* dst, size_t dst_stride) {
    int ow = 0, oh = 0;
    if (!bgr || !dst || poppy_frame_scaled_size(width, height, factor, &ow, &oh) != POPPY_OK) return POPPY_E_ARG;
    if (stride < (size_t)width * 3 || dst_stride < (size_t)ow * 3) return POPPY_E_ARG;
    const int s = factor;
    for (int y = 0; y < oh; ++y) {
        const int y0 = y * s, ny = y0 + s <= height ? s : height - y0;
        uint8_t* o = dst + (size_t)y * dst_stride;
        for (int x = 0; x < ow; ++x) {
            const int x0 = x * s, nx = x0 + s <= width ? s : width - x0, n = nx * ny;
            int sum[3] = {0, 0, 0};
            for (int r = 0; r < ny; ++r) {
                const uint8_t* p = bgr + (size_t)(y0 + r) * stride + (size_t)x0 * 3;
                for (int q = 0; q < nx; ++q) { sum[0] += p[3 * q]; sum[1] += p[3 * q + 1]; sum[2] += p[3 * q + 2]; }
            }
            for (int ch = 0; ch < 3; ++ch) o[3 * x + ch] = (uint8_t)((sum[ch] + n / 2) / n);
        }
    }
    return POPPY_OK;
}

}  // extern "C"
