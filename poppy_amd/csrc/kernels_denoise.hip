// kernels_denoise.hip — the non-local-means denoise on the GPU (the rule: include/poppy_hip.h, poppy_bgr_denoise; what both sides share: denoise.h).
// All integer: the float rules of this code base are not in play.  One launch:
//   k_denoise<TW, LDS_TABLE>   a workgroup of 4 waves per 58 x 64 output tile.  The extended tile — (64 + 2 sh) x (64 + 2 th + 2 sh) pixels, every
//                              coordinate folded by reflect-101 as often as needed — is staged once in LDS as one packed dword per pixel (at most 84 x 90
//                              dwords, 30 KB), and beside it the non-zero prefix t[0 .. L) of the weight table when L <= kTableLds (32 KB); a longer prefix
//                              is read from global memory (LDS_TABLE = false).  Wave v takes rows 16 v .. 16 v + 15 of the tile, a lane per column, and
//                              keeps est[3] and ws of its 16 pixels in 64 registers.  Per offset (dx, dy): lane l holds the squared differences of image
//                              column x0 - th + l summed over the template's tw rows, which slides down the 16 rows (add the entering row, subtract the
//                              leaving one); the template's horizontal sum takes lanes l .. l + tw - 1, so lanes 0 .. 57 have a D, for image column x0 + l;
//                              then the shift, the table read (an index at or above L reads nothing) and four multiply-adds.
// The squared distance of two packed pixels is p.p + q.q - 2 p.q with three byte dot products (exact: every term is below 2^18).
#include <hip/hip_runtime.h>
#define POPPY_DENOISE_HD __host__ __device__
#include "denoise.h"
#include "kernels.h"

namespace poppy_hip {

namespace {

using namespace poppy_denoise;

constexpr int kThreads = kWaves * 64;
static_assert(kTileW + kMaxTemplate - 1 == 64, "lane l + tw - 1 stays inside the wave for every lane that has an output");
static_assert((kExtW * kExtH + kTableLds) * 4 <= 64 * 1024, "tile and table fit a workgroup's static LDS");

struct DenoiseArgs {
    const uint8_t* src; size_t stride; uint8_t* dst;       // dst: tight rows
    int w, h, sh, shift; uint32_t L; const uint32_t* table;
};

__device__ inline uint32_t sqdist(uint32_t p, uint32_t q) {
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_udot4)
    const uint32_t s = __builtin_amdgcn_udot4(q, q, __builtin_amdgcn_udot4(p, p, 0u, false), false);
    return s - 2u * __builtin_amdgcn_udot4(p, q, 0u, false);
#else
    const int d0 = (int)(p & 255u) - (int)(q & 255u), d1 = (int)((p >> 8) & 255u) - (int)((q >> 8) & 255u), d2 = (int)(p >> 16) - (int)(q >> 16);
    return (uint32_t)(d0 * d0 + d1 * d1 + d2 * d2);
#endif
}

// (est + s / 2) / s.  est <= 255 s < 2^32, but est + s / 2 passes 2^32 on bright flat images at the widest search (the host statement forms it in 64 bits);
// here: est = q s + r with r < s, and the quotient is q + 1 exactly when r + s / 2 >= s — r + s / 2 < 1.5 s < 2^32
__device__ inline uint8_t rounded_quotient(uint32_t est, uint32_t s) {
    const uint32_t q = est / s, r = est - q * s;
    return (uint8_t)(q + (r + (s >> 1) >= s ? 1u : 0u));
}

template <int TW, bool LDS_TABLE>
__global__ void __launch_bounds__(kThreads) k_denoise(DenoiseArgs a) {
    constexpr int TH = TW / 2;
    __shared__ uint32_t tile[kExtW * kExtH];
    __shared__ uint32_t tab[LDS_TABLE ? kTableLds : 1];
    const int sh = a.sh, b = TH + sh;
    const int EW = 64 + 2 * sh, EH = kTileH + 2 * b;           // <= kExtW, kExtH: sh <= 10, TH <= 3
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    // tile (ex, ey) = image (x0 - b + ex, y0 - b + ey), folded: every read lies inside the image
    for (int i = threadIdx.x; i < EW * EH; i += kThreads) {
        const int ey = i / EW, ex = i - ey * EW;
        const uint8_t* p = a.src + (size_t)fold101(y0 - b + ey, a.h) * a.stride + (size_t)fold101(x0 - b + ex, a.w) * 3;
        tile[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
    if (LDS_TABLE)
        for (uint32_t i = threadIdx.x; i < a.L; i += kThreads) tab[i] = a.table[i];          // L <= kTableLds (launch_denoise)
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // lane l sums image column x0 - TH + l = tile column l + sh; its output is image column x0 + l = tile column l + b (lanes below kTileW)
    const int out_lane = lane < kTileW ? lane : 0;             // the other lanes accumulate nothing that is stored; they stay inside the tile
    const uint32_t* pc = tile + (wave * kWaveRows + sh) * EW + lane + sh;          // row 0 of the template of the wave's row 0
    const uint32_t* qa0 = tile + (wave * kWaveRows + b) * EW + out_lane + b;       // the wave's row 0 at offset (0, 0)
    uint32_t e0[kWaveRows], e1[kWaveRows], e2[kWaveRows], ws[kWaveRows];
#pragma unroll
    for (int r = 0; r < kWaveRows; ++r) e0[r] = e1[r] = e2[r] = ws[r] = 0u;

    for (int dy = -sh; dy <= sh; ++dy)
        for (int dx = -sh; dx <= sh; ++dx) {
            // rows: wave * 16 + sh + dy + (0 .. 15 + TW - 1) lies in 0 .. EH - 1; columns: lane + sh + dx in 0 .. 63 + 2 sh = EW - 1
            const uint32_t* qc = pc + dy * EW + dx;
            const uint32_t* qa = qa0 + dy * EW + dx;           // column out_lane + b + dx <= 57 + TH + 2 sh < EW, row <= 63 + b + sh < EH
            uint32_t V = 0;
#pragma unroll
            for (int j = 0; j < TW; ++j) V += sqdist(pc[j * EW], qc[j * EW]);
#pragma unroll
            for (int r = 0; r < kWaveRows; ++r) {
                if (r > 0) V += sqdist(pc[(r + TW - 1) * EW], qc[(r + TW - 1) * EW]) - sqdist(pc[(r - 1) * EW], qc[(r - 1) * EW]);
                uint32_t D = V;
#pragma unroll
                for (int i = 1; i < TW; ++i) D += (uint32_t)__shfl_down((int)V, i);          // lanes above 57 get sums nobody stores
                const uint32_t idx = D >> a.shift;
                uint32_t wgt = 0u;
                if (idx < a.L) wgt = LDS_TABLE ? tab[idx] : a.table[idx];
                const uint32_t q = qa[r * EW];
                e0[r] += wgt * (q & 255u); e1[r] += wgt * ((q >> 8) & 255u); e2[r] += wgt * (q >> 16);
                ws[r] += wgt;
            }
        }

    const int x = x0 + lane;
    if (lane >= kTileW || x >= a.w) return;
#pragma unroll
    for (int r = 0; r < kWaveRows; ++r) {
        const int y = y0 + wave * kWaveRows + r;
        if (y >= a.h) break;
        uint8_t* o = a.dst + ((size_t)y * a.w + x) * 3;
        const uint32_t s = ws[r];                              // >= t[0] > 0
        o[0] = rounded_quotient(e0[r], s);
        o[1] = rounded_quotient(e1[r], s);
        o[2] = rounded_quotient(e2[r], s);
    }
}

template <int TW> void launch_tw(const DenoiseArgs& a, dim3 grid, hipStream_t s) {
    if (a.L <= (uint32_t)kTableLds) hipLaunchKernelGGL((k_denoise<TW, true>), grid, dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((k_denoise<TW, false>), grid, dim3(kThreads), 0, s, a);
}

}  // namespace

// src (w x h, rows of `stride` bytes, device) -> dst (tight rows, device) on stream s.  d_table: at least L entries of the table poppy_denoise_weights
// formed for (hs, tw, sw); shift: its shift.  The caller has made the refusals (denoise.h: check_params); the windows are checked again here because the
// kernel's LDS is sized by them.
hipError_t launch_denoise(const uint8_t* src, size_t stride, uint8_t* dst, int w, int h, int tw, int sw, int shift, int L, const uint32_t* d_table, hipStream_t s) {
    if (!src || !dst || !d_table || w <= 0 || h <= 0 || stride < (size_t)w * 3 || L < 1 || L > kMaxTable || shift < 0 || shift > 6) return hipErrorInvalidValue;
    if (tw % 2 == 0 || sw % 2 == 0 || tw < kMinWindow || tw > kMaxTemplate || sw < kMinWindow || sw > kMaxSearch) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((w + kTileW - 1) / kTileW), (unsigned)((h + kTileH - 1) / kTileH));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    const DenoiseArgs a{src, stride, dst, w, h, sw / 2, shift, (uint32_t)L, d_table};
    if (tw == 3) launch_tw<3>(a, grid, s);
    else if (tw == 5) launch_tw<5>(a, grid, s);
    else launch_tw<7>(a, grid, s);
    return hipGetLastError();
}

}  // namespace poppy_hip
