// kernels_frame_scale.hip — the frame a slot rendered (tight u8x3 BGR, w x h) -> the same frame scaled down by a whole factor s (tight, ow x oh,
// ow = (w + s - 1) / s, oh = (h + s - 1) / s) for the writer hand-off (include/poppy_hip.h: poppy_hip_set_frame_scale).  Output pixel (x, y) is the
// rounded mean of source columns [s x, min(s x + s, w)) and rows [s y, min(s y + s, h)): per channel (sum + n / 2) / n over the n pixels covered.
// poppy_bgr_downscale (frame_scale.cpp) is the host statement of the same arithmetic.
//
// Byte work bound by HBM: 3 B/px read, 3 / s^2 B/px written.  The wide kernel (s = 2, 4, 8) takes s rows x 8 source pixels per thread: 3 x 8-byte loads
// per row, 8 / s output pixels stored as three words of 8 / s bytes.  It needs rows that start on 8-byte boundaries (w % 8 == 0, so no block is clipped
// on the right; an 8-byte aligned source) and a destination aligned to its store width.  Every other factor, width and alignment, and the clipped
// bottom row behind the wide kernel, go through the bytewise kernel, one thread per output pixel.
#include "kernels.h"
#include <hip/hip_ext.h>

namespace poppy_hip {

// blocks of 8 x S source pixels over rows [0, S * (h / S)); w % 8 == 0
template <int S>
__global__ void __launch_bounds__(256) k_bgr_downscale(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int bx_n, size_t n_blocks) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_blocks) return;
    const size_t by = t / (size_t)bx_n;
    const int bx = (int)(t - by * (size_t)bx_n);
    constexpr int kOut = 8 / S;                    // output pixels of this thread
    uint32_t sum[kOut][3] = {};
    #pragma unroll
    for (int r = 0; r < S; ++r) {
        const uint2* p = (const uint2*)(src + ((by * S + r) * (size_t)w + (size_t)bx * 8) * 3);
        uint32_t words[6];                         // the row's 24 bytes, as six little-endian words
        #pragma unroll
        for (int k = 0; k < 3; ++k) { const uint2 v = p[k]; words[2 * k] = v.x; words[2 * k + 1] = v.y; }
        #pragma unroll
        for (int i = 0; i < 8; ++i)
            #pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int o = 3 * i + ch;          // byte o of the row's 24
                sum[i / S][ch] += (words[o >> 2] >> (8 * (o & 3))) & 0xffu;
            }
    }
    uint8_t out[3 * kOut];
    #pragma unroll
    for (int j = 0; j < kOut; ++j)
        #pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[3 * j + ch] = (uint8_t)((sum[j][ch] + S * S / 2) / (S * S));
    uint8_t* q = dst + (by * (size_t)(w / S) + (size_t)bx * kOut) * 3;
    if constexpr (S == 2) {                        // 12 bytes on a 4-byte boundary
        #pragma unroll
        for (int k = 0; k < 3; ++k)
            ((uint32_t*)q)[k] = (uint32_t)out[4 * k] | (uint32_t)out[4 * k + 1] << 8 | (uint32_t)out[4 * k + 2] << 16 | (uint32_t)out[4 * k + 3] << 24;
    } else if constexpr (S == 4) {                 // 6 bytes on a 2-byte boundary
        #pragma unroll
        for (int k = 0; k < 3; ++k) ((uint16_t*)q)[k] = (uint16_t)(out[2 * k] | out[2 * k + 1] << 8);
    } else {
        #pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = out[k];
    }
}

// one thread per output pixel (its block clipped at the right and bottom edges) of output rows [oy0, oh)
__global__ void __launch_bounds__(256) k_bgr_downscale_bytes(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h, int s, int ow, int oy0, size_t n_px) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_px) return;
    const size_t row = t / (size_t)ow;
    const int oy = oy0 + (int)row, ox = (int)(t - row * (size_t)ow);
    const int x0 = ox * s, y0 = oy * s;
    const int nx = min(s, w - x0), ny = min(s, h - y0);
    uint32_t sb = 0, sg = 0, sr = 0;
    for (int r = 0; r < ny; ++r) {
        const uint8_t* p = src + ((size_t)(y0 + r) * w + x0) * 3;
        for (int q = 0; q < nx; ++q) { sb += p[3 * q]; sg += p[3 * q + 1]; sr += p[3 * q + 2]; }
    }
    const uint32_t n = (uint32_t)(nx * ny);
    uint8_t* o = dst + ((size_t)oy * ow + ox) * 3;
    o[0] = (uint8_t)((sb + n / 2) / n);
    o[1] = (uint8_t)((sg + n / 2) / n);
    o[2] = (uint8_t)((sr + n / 2) / n);
}

bool bgr_downscale_wide(const uint8_t* src, const uint8_t* dst, int w, int h, int s) {
    if ((s != 2 && s != 4 && s != 8) || w % 8 != 0 || h < s || ((uintptr_t)src & 7) != 0) return false;
    return ((uintptr_t)dst & (uintptr_t)(s == 2 ? 3 : s == 4 ? 1 : 0)) == 0;
}

void launch_bgr_downscale(const uint8_t* src, uint8_t* dst, int w, int h, int s, hipStream_t stream, hipEvent_t done) {
    const int ow = (w + s - 1) / s, oh = (h + s - 1) / s;
    const bool wide = bgr_downscale_wide(src, dst, w, h, s);
    const int wide_rows = wide ? h / s : 0;                       // output rows the wide kernel writes
    const bool tail = wide_rows < oh;
    if (wide) {
        const int bx_n = w / 8;
        const size_t n = (size_t)bx_n * wide_rows;
        const dim3 grid((unsigned)((n + 255) / 256));
        hipEvent_t ev = tail ? nullptr : done;
        if (s == 2) hipExtLaunchKernelGGL(k_bgr_downscale<2>, grid, dim3(256), 0, stream, nullptr, ev, 0, src, dst, w, bx_n, n);
        else if (s == 4) hipExtLaunchKernelGGL(k_bgr_downscale<4>, grid, dim3(256), 0, stream, nullptr, ev, 0, src, dst, w, bx_n, n);
        else hipExtLaunchKernelGGL(k_bgr_downscale<8>, grid, dim3(256), 0, stream, nullptr, ev, 0, src, dst, w, bx_n, n);
    }
    if (tail) {
        const size_t n = (size_t)ow * (oh - wide_rows);
        hipExtLaunchKernelGGL(k_bgr_downscale_bytes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, nullptr, done, 0, src, dst, w, h, s, ow, wide_rows, n);
    }
}

}  // namespace poppy_hip
