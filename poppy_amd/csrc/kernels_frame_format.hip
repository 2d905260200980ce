// kernels_frame_format.hip — the frame a slot rendered (tight u8x3 BGR) -> I420 for the writer hand-off (include/poppy_hip.h:
// poppy_hip_set_frame_format).  Full-range BT.601 with 16 fractional bits, chroma of each 2 x 2 block from its channel sums;
// poppy_bgr_to_i420 (frame_sink.cpp) is the host statement of the same arithmetic, and the Y plane is the C444 sink's.
//
// Byte work bound by HBM: 3 B/px read, 1.5 B/px written.  The wide kernel takes 2 rows x 8 pixels per thread: 3 x 8-byte loads per row,
// one 8-byte Y store per row, one 4-byte U and one 4-byte V store.  It needs rows that start on 8-byte boundaries (width % 8 == 0, 8-byte aligned buffers);
// every other width, and the last row of an odd height, go through the tail kernel, one thread per 2 x 2 block with byte accesses.
#include "kernels.h"
#include <hip/hip_ext.h>

namespace poppy_hip {

__device__ __forceinline__ int clamp_u8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
__device__ __forceinline__ int luma(int b, int g, int r) { return clamp_u8((19595 * r + 38470 * g + 7471 * b + 32768) >> 16); }
// k = log2 of the pixels summed (0, 1, 2); >> of a negative int is arithmetic on this target
__device__ __forceinline__ int chroma_u(int sb, int sg, int sr, int k) { return clamp_u8(((-11059 * sr - 21709 * sg + 32768 * sb + (32768 << k)) >> (16 + k)) + 128); }
__device__ __forceinline__ int chroma_v(int sb, int sg, int sr, int k) { return clamp_u8(((32768 * sr - 27439 * sg - 5329 * sb + (32768 << k)) >> (16 + k)) + 128); }

// blocks of 8 x 2 pixels over rows [0, 2 * (h / 2)); w % 8 == 0
__global__ void __launch_bounds__(256) k_bgr_to_i420(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h, int bx_n, int n_blocks) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_blocks) return;
    const int by = t / bx_n, bx = t - by * bx_n;
    const int x = bx * 8, y = by * 2;
    const int cw = w >> 1, ch = (h + 1) >> 1;
    uint32_t words[2][6];                          // the 24 bytes of each row, as six little-endian words
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint2* p = (const uint2*)(src + ((size_t)(y + r) * w + x) * 3);
        #pragma unroll
        for (int k = 0; k < 3; ++k) { const uint2 v = p[k]; words[r][2 * k] = v.x; words[r][2 * k + 1] = v.y; }
    }
    uint32_t yw[2][2] = {{0, 0}, {0, 0}};
    uint32_t uw = 0, vw = 0;
    #pragma unroll
    for (int j = 0; j < 4; ++j) {                  // chroma sample j: pixels 2j, 2j + 1 of both rows
        int sb = 0, sg = 0, sr = 0;
        #pragma unroll
        for (int r = 0; r < 2; ++r)
            #pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int i = 2 * j + q;
                auto at = [&](int o) { return (int)((words[r][o >> 2] >> (8 * (o & 3))) & 0xffu); };      // byte o of the row's 24
                const int b = at(3 * i), g = at(3 * i + 1), rr = at(3 * i + 2);
                sb += b; sg += g; sr += rr;
                yw[r][i >> 2] |= (uint32_t)luma(b, g, rr) << (8 * (i & 3));
            }
        uw |= (uint32_t)chroma_u(sb, sg, sr, 2) << (8 * j);
        vw |= (uint32_t)chroma_v(sb, sg, sr, 2) << (8 * j);
    }
    #pragma unroll
    for (int r = 0; r < 2; ++r) *(uint2*)(dst + (size_t)(y + r) * w + x) = make_uint2(yw[r][0], yw[r][1]);
    uint8_t* u = dst + (size_t)w * h;
    const size_t ci = (size_t)by * cw + (x >> 1);
    *(uint32_t*)(u + ci) = uw;
    *(uint32_t*)(u + (size_t)cw * ch + ci) = vw;
}

// one thread per 2 x 2 block (clipped at the right and bottom edges) of chroma rows [cy0, ch)
__global__ void __launch_bounds__(256) k_bgr_to_i420_tail(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h, int cy0, int n_blocks) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_blocks) return;
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1;
    const int cy = cy0 + t / cw, cx = t % cw;
    const int x0 = 2 * cx, y0 = 2 * cy;
    const int nx = x0 + 1 < w ? 2 : 1, ny = y0 + 1 < h ? 2 : 1;
    int sb = 0, sg = 0, sr = 0;
    for (int r = 0; r < ny; ++r)
        for (int q = 0; q < nx; ++q) {
            const size_t o = (size_t)(y0 + r) * w + x0 + q;
            const int b = src[3 * o], g = src[3 * o + 1], rr = src[3 * o + 2];
            sb += b; sg += g; sr += rr;
            dst[o] = (uint8_t)luma(b, g, rr);
        }
    const int k = (nx >> 1) + (ny >> 1);
    uint8_t* u = dst + (size_t)w * h;
    const size_t ci = (size_t)cy * cw + cx;
    u[ci] = (uint8_t)chroma_u(sb, sg, sr, k);
    u[(size_t)cw * ch + ci] = (uint8_t)chroma_v(sb, sg, sr, k);
}

void launch_bgr_to_i420(const uint8_t* src, uint8_t* dst, int w, int h, hipStream_t s, hipEvent_t done) {
    const int ch = (h + 1) / 2;
    const bool wide = w % 8 == 0 && h >= 2 && (((uintptr_t)src | (uintptr_t)dst) & 7) == 0;
    const int wide_rows = wide ? h / 2 : 0;                      // chroma rows the wide kernel writes
    const bool tail = wide_rows < ch;
    if (wide) {
        const int bx_n = w / 8, n = bx_n * wide_rows;
        hipExtLaunchKernelGGL(k_bgr_to_i420, dim3((n + 255) / 256), dim3(256), 0, s, nullptr, tail ? nullptr : done, 0, src, dst, w, h, bx_n, n);
    }
    if (tail) {
        const int n = ((w + 1) / 2) * (ch - wide_rows);
        hipExtLaunchKernelGGL(k_bgr_to_i420_tail, dim3((n + 255) / 256), dim3(256), 0, s, nullptr, done, 0, src, dst, w, h, wide_rows, n);
    }
}

}  // namespace poppy_hip
