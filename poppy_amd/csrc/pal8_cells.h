// pal8_cells.h — what the kernels that read BGR pixels through a cell -> index table share (kernels_frame_pal8.hip: k_pal8_hist, k_pal8_seq_pass, k_pal8_remap;
// kernels_frame_gif.hip: k_gif_lzw_bgr): a pixel's cell among the 32^3, and four pixels read as three words.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace poppy_hip {
namespace {

__device__ __forceinline__ int cell_of(int b, int g, int r) { return ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3); }

// the (up to) four pixels of quad q as 12 bytes in three words; n = how many of them exist
__device__ __forceinline__ void load_quad(const uint8_t* __restrict__ src, size_t q, int n, bool aligned, uint32_t w[3]) {
    if (aligned && n == 4) {
        const uint32_t* p = (const uint32_t*)(src + q * 12);
        w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
    } else {
        w[0] = w[1] = w[2] = 0;
        #pragma unroll
        for (int i = 0; i < 12; ++i) if (i < 3 * n) w[i >> 2] |= (uint32_t)src[q * 12 + i] << (8 * (i & 3));
    }
}
__device__ __forceinline__ int quad_byte(const uint32_t w[3], int o) { return (int)((w[o >> 2] >> (8 * (o & 3))) & 0xffu); }

}  // namespace
}  // namespace poppy_hip
