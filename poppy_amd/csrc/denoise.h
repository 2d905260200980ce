// denoise.h — non-local-means denoising of an 8-bit BGR image with one strength (the rule: include/poppy_hip.h, poppy_bgr_denoise).  The host statement
// (denoise.cpp) and the kernel (kernels_denoise.hip) are pinned to each other with ==.  What both sides must agree on is here: the windows that exist, the
// reflect-101 fold, and the kernel's geometry, which the tests read through poppy_denoise_tile and poppy_denoise_table_bound instead of copying it.
// The weight table and its constants are formed in ONE place, poppy_denoise_weights (denoise.cpp); the GPU path uploads what that returns.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef POPPY_DENOISE_HD
#define POPPY_DENOISE_HD
#endif

namespace poppy_denoise {

constexpr int kMinWindow = 3, kMaxTemplate = 7, kMaxSearch = 21;      // odd windows: template 3..7, search 3..21
constexpr int kMaxDist = 3 * 255 * 255;                               // 195075: the largest squared distance of two BGR pixels
constexpr int kMaxTable = kMaxDist + 1;                               // no table is longer (mult >= 1)

// The kernel's geometry (kernels_denoise.hip): a workgroup of kWaves waves per kTileW x kTileH output tile, a lane per column, a wave per kWaveRows rows.
// A wave's 64 lanes hold the column sums of 64 neighbouring columns; the template's horizontal sum takes tw of them, so 64 - (kMaxTemplate - 1) lanes
// have an output.
constexpr int kTileW = 64 - (kMaxTemplate - 1), kWaveRows = 16, kWaves = 4, kTileH = kWaveRows * kWaves;
constexpr int kExtW = 64 + (kMaxSearch - 1), kExtH = kTileH + (kMaxTemplate - 1) + (kMaxSearch - 1);      // the staged tile at the largest windows, in pixels
// The non-zero prefix t[0 .. L) of the weight table is staged in LDS beside the tile when L is at most this; longer prefixes are read from global memory.
// 30 KB of tile + 32 KB of table: two workgroups per CU's 160 KiB.
constexpr int kTableLds = 8192;

// reflect-101, folded as often as needed: i may lie any distance outside 0 .. n - 1; a side of 1 maps every index to 0
POPPY_DENOISE_HD inline int fold101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// ---- host side (denoise.cpp) ---------------------------------------------------------------------------------------------------------------------------
// POPPY_OK, POPPY_E_ARG (hs not finite or <= 0, an even or non-positive window) or POPPY_E_UNSUPPORTED (a window that does not exist): the refusal every
// entry point makes, in this order, with *why (may be null) naming it
int check_params(float hs, int tw, int sw, const char** why);

}  // namespace poppy_denoise
