// kernels_frame_resize.hip — the frame a slot rendered (tight u8x3 BGR, w x h) -> the same frame resampled to ow x oh (tight) by exact area weights, for the
// writer hand-off (include/poppy_hip.h: poppy_hip_set_frame_size).  Output pixel (x, y), per channel:
//    (sum over r, i of wy(y, r) wx(x, i) src(i, r) + w h / 2) / (w h),   wx(x, i) = |[x w, (x + 1) w) ∩ [i ow, (i + 1) ow)|,  wy likewise with h and oh.
// poppy_bgr_resize_area (frame_resize.cpp) is the host statement of the same arithmetic; nothing here is floating point.
//
// One thread per output pixel, reading its source pixels from global memory byte by byte.  A form that staged the source footprint of 64 x 4 output pixels in LDS
// with aligned 16-byte loads was built and measured: it did not win at 1080p -> 1280 x 720 ("Resized hand-off"), so this is the only form.
// The kernel comes in three widths of arithmetic, chosen by the launcher from the sizes alone (bgr_resize_area_form):
//    2  32-bit sums and 32-bit indices: w h <= 2^24 (the numerator is at most 255.5 w h < 2^32) and w, h <= 32768 (every index product is at most w^2 <= 2^30)
//    1  32-bit sums, 64-bit indices: w h <= 2^24 with a side above 32768
//    0  64-bit sums and indices: frames above 2^24 pixels
#include "kernels.h"
#include <hip/hip_ext.h>

namespace poppy_hip {

constexpr unsigned kResizeMaxSide32 = 32768;
constexpr unsigned long long kResize32BitPixels = 1ull << 24;

template <typename Sum, typename Idx>
__global__ void __launch_bounds__(256) k_bgr_resize_area(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, unsigned w, unsigned h, unsigned ow, unsigned oh,
                                                         size_t n_px) {
    const size_t t64 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t64 >= n_px) return;
    const Idx t = (Idx)t64;                                         // (form 2: n_px <= w h <= 2^24)
    const Idx y = t / ow, x = t - y * ow;
    const Idx xa = x * w, xb = xa + w, ya = y * h, yb = ya + h;     // the pixel's extent in 1 / ow columns and 1 / oh rows
    const Idx i0 = xa / ow, i1 = (xb - 1) / ow, q0 = ya / oh, q1 = (yb - 1) / oh;
    Sum sb = 0, sg = 0, sr = 0;
    for (Idx q = q0; q <= q1; ++q) {
        const Sum wy = (Sum)(min((q + 1) * oh, yb) - max(q * oh, ya));
        const uint8_t* px = src + ((size_t)q * w + i0) * 3;
        Sum b = 0, g = 0, rr = 0;
        for (Idx i = i0; i <= i1; ++i, px += 3) {
            const Sum wx = (Sum)(min((i + 1) * ow, xb) - max(i * ow, xa));
            b += wx * px[0]; g += wx * px[1]; rr += wx * px[2];
        }
        sb += wy * b; sg += wy * g; sr += wy * rr;
    }
    const Sum area = (Sum)w * (Sum)h, half = area / 2;
    uint8_t* o = dst + t64 * 3;
    o[0] = (uint8_t)((sb + half) / area);
    o[1] = (uint8_t)((sg + half) / area);
    o[2] = (uint8_t)((sr + half) / area);
}

int bgr_resize_area_form(int w, int h, int ow, int oh) {
    (void)ow; (void)oh;
    if ((unsigned long long)w * (unsigned long long)h > kResize32BitPixels) return 0;
    return (unsigned)w <= kResizeMaxSide32 && (unsigned)h <= kResizeMaxSide32 ? 2 : 1;
}

void launch_bgr_resize_area(const uint8_t* src, uint8_t* dst, int w, int h, int ow, int oh, hipStream_t stream, hipEvent_t done) {
    const unsigned W = (unsigned)w, H = (unsigned)h, OW = (unsigned)ow, OH = (unsigned)oh;
    const size_t n = (size_t)OW * OH;
    const dim3 grid((unsigned)((n + 255) / 256));
    const int form = bgr_resize_area_form(w, h, ow, oh);
    if (form == 2) hipExtLaunchKernelGGL((k_bgr_resize_area<uint32_t, uint32_t>), grid, dim3(256), 0, stream, nullptr, done, 0, src, dst, W, H, OW, OH, n);
    else if (form == 1) hipExtLaunchKernelGGL((k_bgr_resize_area<uint32_t, unsigned long long>), grid, dim3(256), 0, stream, nullptr, done, 0, src, dst, W, H, OW, OH, n);
    else hipExtLaunchKernelGGL((k_bgr_resize_area<unsigned long long, unsigned long long>), grid, dim3(256), 0, stream, nullptr, done, 0, src, dst, W, H, OW, OH, n);
}

}  // namespace poppy_hip
