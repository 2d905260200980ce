// kernels_frame_i444.hip — a frame on the device (tight u8x3 BGR) -> its I444 planes, which the POPPY_FRAME_JPEG444 coder reads (include/poppy_hip.h has the
// rule): three tight w x h planes, Y, U, V, every sample from its own pixel.  poppy_bgr_to_i444 (frame_i444.cpp) is the host statement of the same arithmetic,
// which is k_bgr_to_i420's (kernels_frame_format.hip) with one pixel per chroma sample.
//
// Byte work bound by HBM: 3 B/px read, 3 B/px written.  The wide kernel takes 8 pixels per thread: three 8-byte loads, one 8-byte store per plane.  It needs
// rows that start on 8-byte boundaries (width % 8 == 0 and 8-byte aligned buffers: then every row of the source and of the three planes does); every other
// width and alignment goes through the bytewise kernel, a pixel per thread.
#include "kernels.h"
#include <hip/hip_ext.h>

namespace poppy_hip {

namespace {

__device__ __forceinline__ int clamp_u8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
__device__ __forceinline__ int luma(int b, int g, int r) { return clamp_u8((19595 * r + 38470 * g + 7471 * b + 32768) >> 16); }
// >> of a negative int is arithmetic on this target
__device__ __forceinline__ int chroma_u(int b, int g, int r) { return clamp_u8(((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128); }
__device__ __forceinline__ int chroma_v(int b, int g, int r) { return clamp_u8(((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128); }

}  // namespace

// groups of 8 pixels in raster order (the frame and the planes are tight, and rows are whole groups); n_px % 8 == 0, both buffers 8-byte aligned
__global__ void __launch_bounds__(256) k_bgr_to_i444(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t n_px, size_t n_groups) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_groups) return;
    const uint2* p = (const uint2*)(src + t * 24);
    uint32_t words[6];                             // the group's 24 bytes, as six little-endian words
    #pragma unroll
    for (int k = 0; k < 3; ++k) { const uint2 v = p[k]; words[2 * k] = v.x; words[2 * k + 1] = v.y; }
    uint32_t yw[2] = {0, 0}, uw[2] = {0, 0}, vw[2] = {0, 0};
    #pragma unroll
    for (int i = 0; i < 8; ++i) {
        auto at = [&](int o) { return (int)((words[o >> 2] >> (8 * (o & 3))) & 0xffu); };      // byte o of the 24
        const int b = at(3 * i), g = at(3 * i + 1), r = at(3 * i + 2);
        yw[i >> 2] |= (uint32_t)luma(b, g, r) << (8 * (i & 3));
        uw[i >> 2] |= (uint32_t)chroma_u(b, g, r) << (8 * (i & 3));
        vw[i >> 2] |= (uint32_t)chroma_v(b, g, r) << (8 * (i & 3));
    }
    uint8_t* o = dst + t * 8;
    *(uint2*)o = make_uint2(yw[0], yw[1]);
    *(uint2*)(o + n_px) = make_uint2(uw[0], uw[1]);
    *(uint2*)(o + 2 * n_px) = make_uint2(vw[0], vw[1]);
}

// one thread per pixel, byte accesses: any width, any alignment
__global__ void __launch_bounds__(256) k_bgr_to_i444_bytes(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t n_px) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_px) return;
    const int b = src[3 * t], g = src[3 * t + 1], r = src[3 * t + 2];
    dst[t] = (uint8_t)luma(b, g, r);
    dst[n_px + t] = (uint8_t)chroma_u(b, g, r);
    dst[2 * n_px + t] = (uint8_t)chroma_v(b, g, r);
}

void launch_bgr_to_i444(const uint8_t* src, uint8_t* dst, int w, int h, hipStream_t s, hipEvent_t done) {
    const size_t n_px = (size_t)w * h;
    const bool wide = w % 8 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 7) == 0;
    if (wide) {
        const size_t n = n_px / 8;
        hipExtLaunchKernelGGL(k_bgr_to_i444, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, nullptr, done, 0, src, dst, n_px, n);
    } else {
        hipExtLaunchKernelGGL(k_bgr_to_i444_bytes, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, s, nullptr, done, 0, src, dst, n_px);
    }
}

}  // namespace poppy_hip
