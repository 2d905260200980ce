// frame_resize.cpp — the host side of the resized hand-off (include/poppy_hip.h: poppy_hip_set_frame_size): the size that fits a box and poppy_bgr_resize_area,
// the library's definition of a frame resampled to a smaller size by exact area weights (kernels_frame_resize.hip computes the same bytes on the device).
#include "frame_limits.h"
#include <algorithm>

extern "C" {

int poppy_frame_fit_size(int width, int height, int max_width, int max_height, int* ow, int* oh) {
    if (width <= 0 || height <= 0 || max_width <= 0 || max_height <= 0 || !ow || !oh) return POPPY_E_ARG;
    long long fw = width, fh = height;
    if (width > max_width || height > max_height) {
        if ((long long)width * max_height >= (long long)height * max_width) {
            fw = max_width; fh = std::max(1LL, ((long long)height * max_width + width / 2) / width);
        } else {
            fh = max_height; fw = std::max(1LL, ((long long)width * max_height + height / 2) / height);
        }
    }
    if (!size_admits(width, height, (int)fw, (int)fh)) return POPPY_E_UNSUPPORTED;
    *ow = (int)fw; *oh = (int)fh;
    return POPPY_OK;
}

// output pixel (x, y): per channel (sum of wy(y, r) wx(x, i) src(i, r) + width height / 2) / (width height); wx(x, i) = the overlap of [x width, (x + 1) width)
// and [i ow, (i + 1) ow), wy likewise with height and oh
int poppy_bgr_resize_area(const uint8_t* bgr, size_t stride, int width, int height, int ow, int oh, uint8_t* dst, size_t dst_stride) {
    if (!bgr || !dst || !size_admits(width, height, ow, oh)) return POPPY_E_ARG;
    if (stride < (size_t)width * 3 || dst_stride < (size_t)ow * 3) return POPPY_E_ARG;
    const long long W = width, H = height, area = W * H;
    for (long long y = 0; y < oh; ++y) {
        const long long r0 = y * H / oh, r1 = ((y + 1) * H - 1) / oh;
        uint8_t* o = dst + (size_t)y * dst_stride;
        for (long long x = 0; x < ow; ++x) {
            const long long i0 = x * W / ow, i1 = ((x + 1) * W - 1) / ow;
            unsigned long long sum[3] = {0, 0, 0};
            for (long long r = r0; r <= r1; ++r) {
                const unsigned long long wy = (unsigned long long)(std::min((r + 1) * oh, (y + 1) * H) - std::max(r * oh, y * H));
                const uint8_t* p = bgr + (size_t)r * stride;
                for (long long i = i0; i <= i1; ++i) {
                    const unsigned long long wgt = wy * (unsigned long long)(std::min((i + 1) * ow, (x + 1) * W) - std::max(i * ow, x * W));
                    for (int ch = 0; ch < 3; ++ch) sum[ch] += wgt * p[3 * i + ch];
                }
            }
            for (int ch = 0; ch < 3; ++ch) o[3 * x + ch] = (uint8_t)((sum[ch] + (unsigned long long)(area / 2)) / (unsigned long long)area);
        }
    }
    return POPPY_OK;
}

}  // extern "C"
