// png_tables.h — the constants of the POPPY_FRAME_PNG hand-off format (include/poppy_hip.h has the rule) that the host statement (frame_png.cpp) and the device
// coder (kernels_frame_png.hip) share: the eight code-length tables over literal 0..255 and end-of-block, each table's deflate block header, the canonical
// codes, the capacity, and the CRC-32 arithmetic.  Host and device, nothing of HIP.
// Written by tools/gen_png_tables.py, which states the construction.  This file is the definition: it is never regenerated silently.
#pragma once
#include "../../include/poppy_hip.h"
#include <cstddef>
#include <cstdint>

namespace poppy_hip {
namespace png {

constexpr int kTables = POPPY_PNG_TABLES, kSymbols = 257, kEob = 256;
constexpr int kHeaderWords = 31;      // the longest header in 32-bit words

// kLen[k][v]: the bits of symbol v under table k
constexpr uint8_t kLen[kTables][kSymbols] = {
    { 1,  3,  5,  7,  9, 10, 13, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 12, 10,  8,  7,  4,  2,
     15},
    { 2,  3,  3,  4,  5,  6,  8,  9, 10, 10, 11, 12, 14, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 14, 13, 12, 11, 10,  9,  8,  7,  6,  5,  4,  3,  3,
     15},
    { 3,  3,  4,  4,  5,  5,  5,  6,  6,  7,  7,  7,  8,  8,  9,  9, 10, 10, 11, 11, 11, 12, 12, 13, 13, 13, 14, 14, 14, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 12, 12, 11, 11, 10, 10, 10,  9,  9,  8,  8,  7,  7,  6,  6,  6,  5,  5,  4,  4,  4,  3,
     15},
    { 4,  4,  4,  5,  5,  5,  5,  5,  5,  6,  6,  6,  6,  6,  7,  7,  7,  7,  8,  8,  8,  8,  8,  8,  9,  9,  9,  9,  9, 10, 10, 10,
     10, 10, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 13, 13, 13, 13, 14, 14, 14, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 14, 14, 14, 14, 14, 13, 13, 13, 13, 13, 12, 12, 12, 12, 12, 11, 11, 11, 11, 11, 10,
     10, 10, 10, 10,  9,  9,  9,  9,  9,  8,  8,  8,  8,  8,  7,  7,  7,  7,  7,  6,  6,  6,  6,  6,  5,  5,  5,  5,  5,  5,  4,  4,
     15},
    { 5,  5,  5,  5,  5,  5,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11,
     11, 11, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 14, 14, 14, 14,
     14, 14, 14, 14, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
     15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 14, 14, 14, 14, 14, 14,
     14, 14, 14, 14, 14, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 11, 11, 11, 11, 11, 11,
     11, 11, 11, 11, 11, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  5,  5,  5,  5,  5,
     15},
    { 6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,
      7,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  9,  9,  9,  9,  9,  9,  9,  9,  9,
      9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
     10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 12, 12, 12, 12, 12, 12, 12,
     13, 12, 12, 12, 12, 12, 12, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 10, 10,
     10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,
      9,  9,  9,  9,  9,  9,  9,  9,  9,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  6,  6,  6,  6,  6,  6,  6,  6,  6,  6,
     13},
    { 7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,
      9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
     11, 10, 10, 10, 10, 10, 10, 10, 10, 10,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,
      9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  9,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,  7,
     11},
    { 9,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,
      9},
};

// the block header of table k: kHeaderBits[k] bits, least significant bit of word 0 first; bit 0 is BFINAL, 0 here
constexpr int kHeaderBits[kTables] = {380, 436, 547, 716, 970, 811, 604, 332};
constexpr uint32_t kHeader[kTables][kHeaderWords] = {
    {0xa001e004u, 0x6594582cu, 0xf9bec4c1u, 0x0000006bu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0xd0000000u, 0x012cf2f5u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0xa001e004u, 0xacb6d96du, 0xad11fce9u, 0xcf33b58fu, 0x000002adu, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0xeef50000u, 0xe8e6bdc9u, 0x0007c22du, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0xa001e004u, 0x26965b6du, 0x18fffce8u, 0xf6b5ce73u, 0xfbdce7deu, 0x5664445eu, 0x00037755u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0xba000000u, 0x23332abbu, 0x9ef77bdeu, 0x6b5af7b3u,
     0xefc631ceu, 0x00000003u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x8001e004u, 0x289a4b6du, 0x1ffffce8u, 0xd6b11111u, 0xbdef6b5au, 0xcf333333u, 0x7bdce739u, 0xaaaaadefu,
     0xef7eeeeeu, 0x199999bdu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x33300000u, 0xf7bdef33u,
     0xaabbbbbau, 0xf7bdeeaau, 0xc9ce739eu, 0xf7bdccccu, 0xb5ad6bdeu, 0xfe222222u, 0x000007dfu, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x8001e004u, 0x20625924u, 0xfffffd56u, 0x111111ffu, 0x99991111u, 0x59999999u, 0x55555555u, 0xdddddd55u,
     0x333dddddu, 0x33333333u, 0xbbbbbbbbu, 0x92492bbbu, 0xeeeee924u, 0xb6ceeeeeu, 0x0036db6du, 0x00000000u,
     0x00000000u, 0x60000000u, 0xfb6db6dbu, 0xeeeeeeeeu, 0x4924924eu, 0xeeeeeed2u, 0xccceeeeeu, 0x4cccccccu,
     0x77777777u, 0x55555777u, 0x66555555u, 0x66666666u, 0x44444446u, 0xfffffc44u, 0x000001e7u},
    {0x4001c004u, 0x30a1071bu, 0xbbbbbbe0u, 0x924bbbbbu, 0x24924924u, 0x00049249u, 0x00000000u, 0xdb6db6dau,
     0xb6db6db6u, 0xdb6db6ddu, 0xb6db6db6u, 0x5555554du, 0x7bdf5555u, 0xbff7bdefu, 0xaa7bdef7u, 0xaaaaaaaau,
     0xdb6db6eau, 0xb6db6db6u, 0xb6db6d6du, 0x6db6db6du, 0x0000005bu, 0x49200000u, 0x92492492u, 0xbb924924u,
     0xbbbbbbbbu, 0x000003ffu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x2001c004u, 0x00028813u, 0xb6db6dd0u, 0x6db6db6du, 0xdb6db6dbu, 0x00000000u, 0xaaaaa000u, 0xaaaaaaaau,
     0xaaaaaaaau, 0xeeeeeeeau, 0xdddfeeeeu, 0x555dddddu, 0x55555555u, 0x55555555u, 0x00001555u, 0xd8000000u,
     0xb6db6db6u, 0x6db6db6du, 0x07fdb6dbu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
    {0x2001c004u, 0x00000010u, 0x000001a0u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000700u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u,
     0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u},
};

constexpr bool kraft_is_one(int k) {
    unsigned sum = 0;
    for (int v = 0; v < kSymbols; ++v) sum += 1u << (15 - kLen[k][v]);
    return sum == 1u << 15;
}
constexpr int longest(int k, int n_symbols) {
    int m = 0;
    for (int v = 0; v < n_symbols; ++v) m = kLen[k][v] > m ? kLen[k][v] : m;
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
constexpr int kL7 = longest(7, 256);                        // table 7's longest literal: what a byte costs at most, since table 7 is always a candidate
static_assert(kL7 <= 9, "the capacity counts 9 bits per byte at most");

// deflate's canonical code of every symbol, bit-reversed (the stream takes a code's most significant bit first, everything is packed from bit 0 up), with its
// length: entry = reversed code << 4 | length
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

// The frame's fixed parts (include/poppy_hip.h: File): `total`, the signature, IHDR, IDAT's length and type, the zlib header; the deflate bits begin at kStreamByte.
// Behind them: Adler-32, IDAT's CRC, IEND.
constexpr size_t kSegment = POPPY_PNG_SEGMENT_BYTES;
constexpr size_t kOffSignature = 4, kOffIhdr = 12, kOffIdat = 37, kOffIdatType = 41, kStreamByte = 47, kTailBytes = 4 + 4 + 12;
constexpr size_t kFrameMinBytes = kStreamByte + 1 + kTailBytes;
constexpr uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
constexpr uint8_t kIend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
// a block of s bytes at its bound in bits, and the frame's capacity (include/poppy_hip.h: Capacity)
constexpr unsigned long long kBlockBitsOver = (unsigned long long)kHeaderBits[7] + kLen[7][kEob];
constexpr unsigned long long kSegmentBitsMax = kBlockBitsOver + (unsigned long long)kL7 * kSegment;
constexpr unsigned long long stream_bytes(unsigned long long w, unsigned long long h) { return h * (1 + 3 * w); }
constexpr unsigned long long segment_count(unsigned long long w, unsigned long long h) { return (stream_bytes(w, h) + kSegment - 1) / kSegment; }
constexpr unsigned long long frame_capacity(unsigned long long w, unsigned long long h) {
    return kStreamByte + (segment_count(w, h) * kBlockBitsOver + (unsigned long long)kL7 * stream_bytes(w, h) + 7) / 8 + kTailBytes;
}

// CRC-32 (the PNG specification's, reflected, polynomial 0xEDB88320) as arithmetic on polynomials over GF(2) modulo the generator, in the reflected form: bit 31
// is x^0.  The raw remainder (register started at 0, no final inversion) of a concatenation is raw(A) * x^(8 |B|) + raw(B), and leading zero bytes change
// nothing; the checksum of an L-byte message is raw + 0xFFFFFFFF * x^(8 L) + 0xFFFFFFFF.  That is what lets the device take the CRC in pieces.
constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = b & 1u ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
struct CrcPowers { uint32_t e[64]; };                       // e[k] = x^(2^k)
constexpr CrcPowers make_crc_powers() {
    CrcPowers t{};
    t.e[0] = 1u << 30;
    for (int k = 1; k < 64; ++k) t.e[k] = crc_mul(t.e[k - 1], t.e[k - 1]);
    return t;
}
constexpr uint32_t crc_x_pow_bytes(unsigned long long n_bytes, const CrcPowers& t) {      // x^(8 n)
    uint32_t p = 1u << 31;
    for (int k = 3; n_bytes; n_bytes >>= 1, ++k) if (n_bytes & 1) p = crc_mul(t.e[k], p);
    return p;
}
struct CrcTable { uint32_t e[256]; };
constexpr CrcTable make_crc_table() {
    CrcTable t{};
    for (uint32_t n = 0; n < 256; ++n) {
        uint32_t c = n;
        for (int k = 0; k < 8; ++k) c = c & 1u ? (c >> 1) ^ kCrcPoly : c >> 1;
        t.e[n] = c;
    }
    return t;
}
constexpr uint32_t kAdlerMod = 65521;

// the host coder (frame_png.cpp): a BGR frame with rows `stride` bytes apart into `dst` (the capacity); returns `total`
size_t encode_bgr(const uint8_t* bgr, size_t stride, int w, int h, uint8_t* dst);

}  // namespace png
}  // namespace poppy_hip
