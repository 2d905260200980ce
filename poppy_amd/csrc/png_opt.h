// png_opt.h — the constants of the POPPY_FRAME_PNG_OPT hand-off format (include/poppy_hip.h has the rule) that the host statement (frame_png_opt.cpp) and the
// device coder (kernels_frame_png.hip) share: the ninth candidate of a segment, its own table (under POPPY_FRAME_PNG_SEQ, frame_png_seq.cpp: its sequence's one table, in the same record); the bounds of an own header; the code-length code's order; what a
// place of the header's length sequence sends.  Everything else is POPPY_FRAME_PNG_RUNS': png_runs_tables.h.  Host and device, nothing of HIP.
#pragma once
#include "png_runs_tables.h"

namespace poppy_hip {
namespace png {
// what the PNG coder's two format-specific steps are (frame_limits.h: FormatTraits::variant; kernels.h: launch_png_*)
enum Variant { kLiterals = 0, kRuns = 1, kRunsOwn = 2, kRunsSeq = 3 };      // POPPY_FRAME_PNG, POPPY_FRAME_PNG_RUNS, POPPY_FRAME_PNG_OPT, POPPY_FRAME_PNG_SEQ
}
namespace png_opt {

using png_runs::kSymbols; using png_runs::kEob; using png_runs::kTables;
constexpr int kOwn = kTables;                               // the choice that names the segment's own table; 0..7 are POPPY_FRAME_PNG_RUNS' tables
constexpr int kLimit = 15, kClLimit = 7, kClSymbols = 19;
constexpr int kSequenceMax = kSymbols + 1;                  // the lit/len lengths and the distance code's 1
constexpr int kOwnHeaderBitsMax = 17 + kClSymbols * 3 + kSequenceMax * 7;      // no sequence entry costs more than 7 bits per length it covers
constexpr int kOwnHeaderWords = (kOwnHeaderBitsMax + 31) / 32;
static_assert(kOwnHeaderBitsMax == 2083 && kOwnHeaderWords == 66, "include/poppy_hip.h states the bound");
// RFC 1951, 3.2.7: the order in which the code-length code's own lengths are sent
constexpr uint8_t kClOrder[kClSymbols] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// What the place `offset` of a maximal run of `run` equal lengths `value` sends in the header's length sequence (include/poppy_hip.h: Block header): symbol < 0
// for a place that an earlier entry covers; else the code-length symbol, and for 16, 17, 18 the extra bits and their value.
struct Entry { int symbol, extra_bits; uint32_t extra; };
constexpr Entry entry_at(int value, int run, int offset) {
    if (value == 0) {
        const int full = run / 138, rem = run - 138 * full, q = offset / 138, r = offset - 138 * q;      // (every remainder in front of a full entry is >= 138 >= 11)
        if (q < full) return r == 0 ? Entry{18, 7, 138 - 11} : Entry{-1, 0, 0};
        if (rem >= 11) return r == 0 ? Entry{18, 7, (uint32_t)(rem - 11)} : Entry{-1, 0, 0};
        if (rem >= 3) return r == 0 ? Entry{17, 3, (uint32_t)(rem - 3)} : Entry{-1, 0, 0};
        return Entry{0, 0, 0};
    }
    if (offset == 0) return Entry{value, 0, 0};             // the length once, then repeats of it
    const int rest = run - 1, full = rest / 6, rem = rest - 6 * full, j = offset - 1, q = j / 6, r = j - 6 * q;
    if (q < full) return r == 0 ? Entry{16, 2, 3} : Entry{-1, 0, 0};
    if (rem >= 3) return r == 0 ? Entry{16, 2, (uint32_t)(rem - 3)} : Entry{-1, 0, 0};
    return Entry{value, 0, 0};
}
static_assert(entry_at(0, 149, 0).extra == 127 && entry_at(0, 149, 138).symbol == 18 && entry_at(0, 149, 138).extra == 0 && entry_at(0, 148, 138).symbol == 17 &&
              entry_at(0, 148, 138).extra == 7 && entry_at(0, 140, 139).symbol == 0 && entry_at(0, 2, 1).symbol == 0 && entry_at(0, 3, 0).symbol == 17 &&
              entry_at(0, 10, 0).extra == 7 && entry_at(0, 11, 0).symbol == 18 && entry_at(0, 11, 5).symbol < 0, "runs of zeros: 18 while 11 or more are left, then 17, then zeros");
static_assert(entry_at(5, 3, 1).symbol == 5 && entry_at(5, 4, 1).symbol == 16 && entry_at(5, 4, 1).extra == 0 && entry_at(5, 7, 1).extra == 3 && entry_at(5, 8, 7).symbol == 5 &&
              entry_at(5, 10, 7).symbol == 16 && entry_at(5, 10, 7).extra == 0 && entry_at(5, 10, 8).symbol < 0, "runs of a length: itself, then 16 while 3 or more are left");

// The table a segment's own candidate leaves in the coder's scratch, and the one table of a POPPY_FRAME_PNG_SEQ sequence: a symbol's entry as png_runs::Codes' (reversed code << 4 | length, 0 without a code), and
// the header's bits, least significant bit of word 0 first, BFINAL 0, zeros behind `header_bits`.
struct OwnTable { uint32_t code[kSymbols], header_bits, header[kOwnHeaderWords + 1]; };      // (+ 1: the word a 64-bit flush may touch behind the last)

// the host coder (frame_png_opt.cpp): a BGR frame with rows `stride` bytes apart into `dst` (POPPY_FRAME_PNG_RUNS' capacity); returns `total`
size_t encode_bgr(const uint8_t* bgr, size_t stride, int w, int h, uint8_t* dst);

}  // namespace png_opt
}  // namespace poppy_hip
