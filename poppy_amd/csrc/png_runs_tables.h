// png_runs_tables.h — the constants of the POPPY_FRAME_PNG_RUNS hand-off format (include/poppy_hip.h has the rule) that the host statement (frame_png_runs.cpp)
// and the device coder (kernels_frame_png.hip) share: the eight code-length tables over literal 0..255, end-of-block and the length symbols 257..285, each
// table's deflate block header, the canonical codes, the tokens of a run, and the capacity.  Everything else of the file is POPPY_FRAME_PNG's: png_tables.h.
// Host and device, nothing of HIP.
// Written by tools/gen_png_tables.py --runs, which states the construction; the length symbols' weights are theta_k^3 (285) and theta_k^6 (257..284).
// This file is the definition: it is never regenerated silently.
#pragma once
#include "png_tables.h"

namespace poppy_hip {
namespace png_runs {

constexpr int kTables = POPPY_PNG_TABLES, kSymbols = 286, kEob = 256, kRunMin = POPPY_PNG_RUN_MIN;
constexpr int kHeaderWords = 15;      // the longest header in 32-bit words

// kLen[k][v]: the bits of symbol v under table k
constexpr uint8_t kLen[kTables][kSymbols] = {
    { 1,  3,  5,  7,  8, 11, 13, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 12, 11,  8,  6,  5,  2,
     15, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12,  6},
    { 2,  3,  4,  5,  6,  7,  8,  9, 10, 10, 11, 12, 14, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 14, 13, 12, 11, 10,  9,  8,  8,  7,  6,  5,  4,  3,
     15,  8,  8,  8,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  5},
    { 4,  4,  5,  5,  5,  6,  6,  7,  7,  7,  8,  8,  8,  9,  9, 10, 10, 11, 11, 11, 12, 12, 13, 13, 13, 14, 14, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 14, 14, 13, 13, 12, 12, 12, 11, 11, 10, 10, 10,  9,  9,  8,  8,  8,  7,  7,  7,  6,  6,  5,  5,  5,  4,
     15,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  5},
    { 5,  5,  5,  5,  6,  6,  6,  6,  7,  7,  7,  7,  7,  7,  8,  8,  8,  8,  8,  9,  9,  9,  9,  9,  9, 10, 10, 10, 10, 11, 11, 11,
     11, 11, 11, 12, 12, 12, 12, 12, 13, 13, 13, 13, 13, 13, 14, 14, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 14, 14, 14, 14, 14, 13, 13, 13, 13, 13, 13, 12, 12, 12, 12, 12, 11, 11,
     11, 11, 11, 10, 10, 10, 10, 10,  9,  9,  9,  9,  9,  9,  8,  8,  8,  8,  8,  7,  7,  7,  7,  7,  6,  6,  6,  6,  6,  5,  5,  5,
     15,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  5},
    { 6,  6,  6,  6,  6,  6,  6,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  9,  9,  9,
      9,  9,  9,  9,  9,  9,  9,  9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 12, 12, 12,
     12, 12, 12, 12, 12, 12, 12, 12, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 12, 12, 12, 12, 12, 12, 12,
     12, 12, 12, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,  9,  9,  9,  9,  9,  9,  9,
      9,  9,  9,  9,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  6,  6,  6,  6,  6,  6,
     15,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6},
    { 6,  6,  6,  6,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,
      9,  9,  9,  9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11,
     11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12,
     13, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11,
     11, 11, 11, 11, 11, 11, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,  9,  9,  9,  9,
      9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  6,  6,  6,
     13,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  6},
    { 7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  9,  9,  9,  9,  9,  9,
      9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,
      9,  9,  9,  9,  9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
     11, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,  9,  9,  9,  9,  9,
      9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,
      9,  9,  9,  9,  9,  9,  9,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,
     11,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7},
    { 9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,
      9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      9,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8},
};

// the block header of table k: kHeaderBits[k] bits, least significant bit of word 0 first; bit 0 is BFINAL, 0 here
constexpr int kHeaderBits[kTables] = {297, 368, 460, 346, 326, 331, 272, 228};
constexpr uint32_t kHeader[kTables][kHeaderWords] = {
    {0x8003e0ecu, 0x6d825105u, 0x5f73ae51u, 0xb6db1fd6u, 0x6db6db6du, 0xdb6db6dbu, 0xb6db6db6u, 0x8cae99edu,
     0x1b6da7bbu, 0x000000b1u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x8003e0ecu, 0xadb6db6du, 0xb6a5fee9u, 0xb5ae623eu, 0x6db3e64fu, 0xdb6db6dbu, 0xb6db6db6u, 0x6db6db6du,
     0x6bd9ef3bu, 0x6ade8c46u, 0x6c311179u, 0x00007dbbu, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x8003e0ecu, 0x20b6cb6cu, 0x11118f6au, 0x55666673u, 0x39f7b5adu, 0x7eeedee7u, 0xdb6db7efu, 0xb6db6db6u,
     0x6db6db6du, 0xebdeb6dbu, 0xb39ef7beu, 0xaaab5ef7u, 0x88ce7332u, 0x6db4ff18u, 0x000007c4u},
    {0xa003e0ecu, 0x28a2bb2du, 0xce8506dau, 0xcd85c9a1u, 0x6fa7cba3u, 0xdb6db6dbu, 0xb6db6db6u, 0x1e5d3d6du,
     0x0e4d2d6du, 0xfc929575u, 0x01a46db2u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0xa003e0ecu, 0x20828b2du, 0x75b78658u, 0xeb3d6bacu, 0xd595691bu, 0x6db6d8c6u, 0x651b56dbu, 0x67adf1a5u,
     0xdb58eb5du, 0xb6d84e0au, 0x00000016u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0xa003c0ecu, 0x20828b23u, 0x276c42d0u, 0x76da36d7u, 0x6f8db3f7u, 0xc763631bu, 0xf1b6f99eu, 0xe36da36cu,
     0x276c46dau, 0x6db1b555u, 0x000001d4u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x6003c0ecu, 0x00020624u, 0xdb63b5c0u, 0x6db393b6u, 0xf6edb5dbu, 0xdb3ddb6bu, 0x6db17db6u, 0xd7fb59dbu,
     0x000035b6u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x6003c0ecu, 0x00000010u, 0xb6db6cb0u, 0x6db6dbadu, 0xdb6db6dbu, 0xb6db6db6u, 0xb6dbab6du, 0x00000006u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
};

constexpr bool kraft_is_one(int k) {
    unsigned sum = 0;
    for (int v = 0; v < kSymbols; ++v) sum += 1u << (15 - kLen[k][v]);
    return sum == 1u << 15;
}
constexpr int longest_literal(int k) {
    int m = 0;
    for (int v = 0; v < 256; ++v) m = kLen[k][v] > m ? kLen[k][v] : m;
    return m;
}
constexpr bool lengths_in_range(int k) {
    for (int v = 0; v < kSymbols; ++v) if (kLen[k][v] < 1 || kLen[k][v] > 15) return false;
    return true;
}
static_assert(kraft_is_one(0) && kraft_is_one(1) && kraft_is_one(2) && kraft_is_one(3) && kraft_is_one(4) && kraft_is_one(5) && kraft_is_one(6) && kraft_is_one(7),
              "every table is a complete prefix code: its Kraft sum is exactly 1");
static_assert(lengths_in_range(0) && lengths_in_range(1) && lengths_in_range(2) && lengths_in_range(3) && lengths_in_range(4) && lengths_in_range(5) &&
              lengths_in_range(6) && lengths_in_range(7), "deflate's codes have 1 to 15 bits");
constexpr int kL7 = longest_literal(7);                     // table 7's longest literal: what a byte costs at most as a literal, since table 7 is always a candidate
static_assert(kL7 <= 9, "the capacity counts 9 bits per byte at most");
static_assert(kHeaderWords * 4 <= POPPY_PNG_HEADER_BYTES, "a header fits the buffer that poppy_png_runs_table fills");

// A match of `length` bytes (3..258) at distance 1 (RFC 1951, 3.2.5): its length symbol, the number of extra bits and their value.  258 is symbol 285.
struct Match { int symbol, extra_bits; uint32_t extra; };
constexpr Match match_of(int length) {
    if (length == 258) return {285, 0, 0};
    const int l = length - 3;
    if (l < 8) return {257 + l, 0, 0};
    int top = 3;
    while (l >> (top + 1)) ++top;
    const int eb = top - 2;
    return {261 + 4 * eb + ((l >> eb) & 3), eb, (uint32_t)l & ((1u << eb) - 1)};
}
constexpr int extra_bits_of_symbol(int s) { return s < 265 || s == 285 ? 0 : (s - 261) / 4; }
// a match costs no more than the three literals it covers at the least, under table 7: its code, its extra bits and the distance code's one bit
constexpr bool matches_within_three_literals() {
    for (int s = 257; s < kSymbols; ++s) if (kLen[7][s] + extra_bits_of_symbol(s) + 1 > 3 * kL7) return false;
    return true;
}
static_assert(matches_within_three_literals(), "the capacity counts a match as the literals it covers");
static_assert(match_of(3).symbol == 257 && match_of(10).symbol == 264 && match_of(11).symbol == 265 && match_of(12).extra == 1 && match_of(257).symbol == 284 &&
              match_of(257).extra == 30 && match_of(257).extra_bits == 5 && match_of(227).symbol == 284 && match_of(226).symbol == 283 && match_of(258).symbol == 285 &&
              match_of(131).symbol == 281 && match_of(130).symbol == 280 && match_of(130).extra == 15, "RFC 1951's length table");

// deflate's canonical code of every symbol, bit-reversed, with its length: entry = reversed code << 4 | length (as png::Codes)
struct Codes { uint32_t e[kTables][kSymbols]; };
constexpr Codes make_codes() {
    Codes c{};
    for (int k = 0; k < kTables; ++k) {
        uint32_t code = 0;
        for (int bits = 1; bits <= 15; ++bits) {
            for (int v = 0; v < kSymbols; ++v) {
                if (kLen[k][v] != bits) continue;
                uint32_t r = 0;
                for (int i = 0; i < bits; ++i) r |= (code >> i & 1u) << (bits - 1 - i);
                c.e[k][v] = r << 4 | (uint32_t)bits;
                ++code;
            }
            code <<= 1;
        }
    }
    return c;
}

// The token that begins at a byte of a run (include/poppy_hip.h: Tokens): the run is `run` bytes, the byte its `offset`-th (0: the run's first).
// Returns 0 for a literal, the match's length for the head of a match, and -(bytes up to the next token) for a byte that a match covers.
constexpr int token_at(int run, int offset) {
    const int m = run - 1;
    if (offset == 0 || m < kRunMin) return 0;
    const int j = offset - 1, q = j / 258, r = j - 258 * q, full = m / 258, rem = m - 258 * full;
    if (q < full) return r == 0 ? 258 : -(258 - r);
    if (rem < 3) return 0;
    return r == 0 ? rem : -(rem - r);
}

using png::kSegment; using png::kStreamByte; using png::kTailBytes; using png::stream_bytes; using png::segment_count;
// a block of s bytes at its bound in bits, and the frame's capacity (include/poppy_hip.h: Capacity)
constexpr unsigned long long kBlockBitsOver = (unsigned long long)kHeaderBits[7] + kLen[7][kEob];
constexpr unsigned long long kSegmentBitsMax = kBlockBitsOver + (unsigned long long)kL7 * kSegment;
constexpr unsigned long long frame_capacity(unsigned long long w, unsigned long long h) {
    return kStreamByte + (segment_count(w, h) * kBlockBitsOver + (unsigned long long)kL7 * stream_bytes(w, h) + 7) / 8 + kTailBytes;
}

// the host coder (frame_png_runs.cpp): a BGR frame with rows `stride` bytes apart into `dst` (the capacity); returns `total`
size_t encode_bgr(const uint8_t* bgr, size_t stride, int w, int h, uint8_t* dst);

}  // namespace png_runs
}  // namespace poppy_hip
