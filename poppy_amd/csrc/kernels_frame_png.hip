// kernels_frame_png.hip — a BGR frame on the device -> POPPY_FRAME_PNG for the writer hand-off (include/poppy_hip.h has the rule; png_tables.h the constants): one
// PNG file whose IDAT is a zlib stream of Huffman-only dynamic blocks, a block per POPPY_PNG_SEGMENT_BYTES of the filtered stream.  poppy_bgr_to_png_frame
// (frame_png.cpp) is the host statement; the bytes are equal.  Nothing in the format is serial but the bit positions and the two checksums, and both combine
// associatively, so the frame is six dispatches on one stream, no host round trip:
//   k_png_filter  a workgroup per row, a thread per pixel (strided) — per four pixels from whole dwords where the width is a multiple of 4 and the frame 4-byte
//                 aligned —: the five filters' scores from the original pixels, a workgroup reduction, the choice (smallest, ties to the lowest type), then
//                 the chosen filter's bytes into the filtered stream in scratch, R, G, B swapped on the way.
//   k_png_cost    a workgroup per segment, 32 bytes per thread: the eight tables' lengths of a byte come from one LDS word (a nibble per table: no length is
//                 above 15), so a segment's eight costs are eight sums; the table (smallest, ties to the lowest), the block's bits, and the segment's Adler
//                 pair: A = the bytes' sum, B = the sum of (len - i) * byte, which is what the segment adds to Adler's b once a is known.
//   k_png_scan    one workgroup: the exclusive prefix sum of the blocks' bits, counted from the FRAME's bit 0 (the deflate bits begin at byte 47, on no word
//                 boundary, and the frame is one bit string), Adler-32 from the pairs (b = n + sum over segments of (bytes behind the segment) * A + B, modulo
//                 65521), and everything that is known now: `total`, the signature, IHDR, IDAT's length and type, the zlib header, Adler-32 and IEND.  It also
//                 stores a zero into every word in which a block begins or the stream ends: the words that two writers share.
//   k_png_pack    a workgroup per segment, the same 32 bytes per thread: a workgroup prefix sum of the threads' code lengths places every thread; a thread
//                 gathers its codes in a 64-bit accumulator that starts at its bit offset inside a word, so that every flush is one whole-word ds_or_b32 into
//                 the block's image in LDS, positioned at the block's start bit mod 32.  The image's words go out as plain stores, except the word the block
//                 begins in and the word it ends in, which its neighbours share: atomicOr on the zeroed word.
//   k_png_crc     IDAT's CRC-32 in pieces: a thread takes 32 bytes counted from the chunk's END (so every piece's distance to the end is known without the
//                 length, and the short piece is the first, where leading zeros change nothing), a table-driven raw remainder, one multiplication by
//                 x^(256 t) modulo the generator, an XOR over the workgroup: a word per 8192 bytes.
//   k_png_finish  one workgroup: the words multiplied into place and XORed, the initial and final inversions, the CRC's four bytes, `total` into the word of
//                 mapped pinned host memory.
// POPPY_FRAME_PNG_RUNS (png_runs_tables.h; poppy_bgr_to_png_runs_frame in frame_png_runs.cpp is its host statement) is the same six dispatches with two kernels
// of its own in the places of k_png_cost and k_png_pack; the filter, the scan, the CRC and the finish are the kernels above, on that format's capacity:
//   k_png_run_cost  the same workgroup per segment and 32 bytes per thread.  A thread marks its breaks (a byte that differs from the one before it, the
//                 segment's first byte, the segment's end) in one 32-bit mask; a forward max-scan of the threads' last breaks and a backward min-scan of their
//                 first breaks over the workgroup tell it where the run of its first byte begins and where the run of its last byte ends.  From a run's start and
//                 length and its own offset every byte decides by itself what it is (png_runs::token_at): a literal, the head of a match, or covered by one.  A
//                 thread counts the tokens that BEGIN in its bytes: eight sums of nibbles from one LDS word per symbol (286 now), and the matches' extra and
//                 distance bits, which are the same under every table.  The Adler pair is a function of the bytes, as before.
//   k_png_run_pack  the same walk again on the chosen table, first for the thread's bit count, then, behind the workgroup's prefix sum, for the bits: a match is
//                 its length code and one more field of extra bits + 1 (the distance code's 0 bit on top), 15 + 6 bits at the most, so the 64-bit
//                 accumulator holds as it does for literals.
// POPPY_FRAME_PNG_OPT (png_opt.h; poppy_bgr_to_png_opt_frame in frame_png_opt.cpp is its host statement) is POPPY_FRAME_PNG_RUNS with two kernels of its own in
// the same two places, and a png_opt::OwnTable per segment behind the scratch's other words:
//   k_png_opt_cost  k_png_run_cost's run bounds and token walk, with the tokens counted into a 286-word LDS histogram (ds_add; end-of-block counts 1): the eight
//                 fixed costs are the histogram's dot products with the nibble table.  Wave 0 then builds the segment's own table while the others leave
//                 (build_code, a lane holds symbols lane + 64 j): the rule's merges in registers as k_jpeg_tables runs them — the two smallest packed keys
//                 (count << 9 | 511 - symbol) by a butterfly of shuffles —, Annex K.3 on lane 0, a symbol's place by (depth, symbol) and then by (length, symbol) as the
//                 number of smaller keys, which give its length and its canonical code.  The header's length sequence: the lanes' break flags are five
//                 ballots, the whole sequence's break mask in every lane, so every place finds its run's start and length by itself and decides what it sends
//                 (png_opt::entry_at, as token_at does for bytes); the 19 counts, the same build at 7 bits, a prefix sum of the entries' bits, and the header
//                 ORed into LDS.  Per segment: the choice 0..8 (8: the own table wins outright; ties go to the fixed tables) and, under 8, the own table.
//   k_png_opt_pack  k_png_run_pack with the codes and the header read from the segment's own table when the choice is 8.  No code is above 15 bits and the block
//                 is no longer than the best fixed table's, so the accumulator and the LDS image hold as they do there.
// POPPY_FRAME_PNG_SEQ (poppy_bgr_frames_to_png_seq_frames in frame_png_seq.cpp is its host statement) is POPPY_FRAME_PNG_OPT with one ninth table per sequence.  A
// frame's place in the sequence store is a POPPY_FRAME_PNG_RUNS scratch; the filter writes the stream there as the frame is rendered, and
//   k_png_seq_count  k_png_opt_cost's histogram of a segment, its non-zero words added (global atomicAdd) to the sequence's 286 sums.
//   k_png_seq_table  once per sequence, one wave: build_code at 15 bits on the sums and the own header, k_png_opt_cost's two routines, into one OwnTable record.
//   k_png_seq_cost   per frame behind the build: k_png_run_cost's walk again with the record's lengths as a ninth column in LDS; the choice 0..8.
//   k_png_seq_pack   k_png_opt_pack with every segment's `own` the sequence's record.
// The scan, the CRC and the finish are the kernels above, on the frame's place.  No launch of these is capped or grid-strided: a workgroup per segment throughout.
// Plain vector stores and atomics only.
#include "kernels.h"
#include <hip/hip_ext.h>

namespace poppy_hip {

namespace {

using namespace png;

constexpr int kThreads = 256, kBytesPerThread = (int)kSegment / kThreads;
static_assert(kBytesPerThread == 32, "a thread takes two 16-byte loads of its segment");
constexpr int kImageWords = (int)((31 + kSegmentBitsMax + 31) / 32) + 1;      // a block at its bound behind 31 bits of offset, and the word a flush may touch
constexpr int kRunImageWords = (int)((31 + png_runs::kSegmentBitsMax + 31) / 32) + 1;
constexpr size_t kCrcBlock = 32 * kThreads;                 // bytes of the chunk per workgroup of k_png_crc
constexpr unsigned long long kFirstBit = 8 * kStreamByte;

struct NibbleTable { uint32_t e[256]; };                    // per literal: table k's length in bits 4 k .. 4 k + 3
constexpr NibbleTable make_nibbles() {
    NibbleTable t{};
    for (int v = 0; v < 256; ++v)
        for (int k = 0; k < kTables; ++k) t.e[v] |= (uint32_t)kLen[k][v] << (4 * k);
    return t;
}
struct RunNibbleTable { uint32_t e[png_runs::kSymbols]; };      // the same per symbol of POPPY_FRAME_PNG_RUNS
constexpr RunNibbleTable make_run_nibbles() {
    RunNibbleTable t{};
    for (int v = 0; v < png_runs::kSymbols; ++v)
        for (int k = 0; k < kTables; ++k) t.e[v] |= (uint32_t)png_runs::kLen[k][v] << (4 * k);
    return t;
}
struct CrcShifts { uint32_t e[kThreads]; };                 // e[t] = x^(8 * 32 * t): what lies behind thread t's piece inside its workgroup
constexpr CrcShifts make_crc_shifts() {
    CrcShifts s{};
    const CrcPowers p = make_crc_powers();
    for (int t = 0; t < kThreads; ++t) s.e[t] = crc_x_pow_bytes(32ull * t, p);
    return s;
}
// e[t] = x^(8 * kCrcBlock * t), what lies behind word t of k_png_crc's output, and stride = x^(8 * kCrcBlock * 256) for the words 256 further on
struct CrcBlockPowers { uint32_t e[kThreads], stride; };
constexpr CrcBlockPowers make_crc_block_powers() {
    CrcBlockPowers s{};
    const CrcPowers p = make_crc_powers();
    for (int t = 0; t < kThreads; ++t) s.e[t] = crc_x_pow_bytes((unsigned long long)kCrcBlock * t, p);
    s.stride = crc_x_pow_bytes((unsigned long long)kCrcBlock * kThreads, p);
    return s;
}
struct HeaderWords { uint32_t e[kTables][kHeaderWords]; };
constexpr HeaderWords make_header_words() {
    HeaderWords h{};
    for (int k = 0; k < kTables; ++k)
        for (int i = 0; i < kHeaderWords; ++i) h.e[k][i] = kHeader[k][i];
    return h;
}
struct BlockOver { uint32_t header[kTables], over[kTables]; };      // H_k, and H_k + len_k[end-of-block]
constexpr BlockOver make_block_over() {
    BlockOver b{};
    for (int k = 0; k < kTables; ++k) { b.header[k] = (uint32_t)kHeaderBits[k]; b.over[k] = (uint32_t)kHeaderBits[k] + kLen[k][kEob]; }
    return b;
}
struct RunHeaderWords { uint32_t e[kTables][png_runs::kHeaderWords]; };
constexpr RunHeaderWords make_run_header_words() {
    RunHeaderWords h{};
    for (int k = 0; k < kTables; ++k)
        for (int i = 0; i < png_runs::kHeaderWords; ++i) h.e[k][i] = png_runs::kHeader[k][i];
    return h;
}
constexpr BlockOver make_run_block_over() {
    BlockOver b{};
    for (int k = 0; k < kTables; ++k) { b.header[k] = (uint32_t)png_runs::kHeaderBits[k]; b.over[k] = (uint32_t)png_runs::kHeaderBits[k] + png_runs::kLen[k][kEob]; }
    return b;
}

struct FixedBytes { uint8_t signature[8], iend[12]; };
constexpr FixedBytes make_fixed_bytes() {
    FixedBytes f{};
    for (int k = 0; k < 8; ++k) f.signature[k] = kSignature[k];
    for (int k = 0; k < 12; ++k) f.iend[k] = kIend[k];
    return f;
}

__constant__ FixedBytes c_fixed = make_fixed_bytes();
__constant__ NibbleTable c_nibbles = make_nibbles();
__constant__ Codes c_codes = make_codes();
__constant__ HeaderWords c_header = make_header_words();
__constant__ BlockOver c_block = make_block_over();
__constant__ RunNibbleTable c_run_nibbles = make_run_nibbles();
__constant__ png_runs::Codes c_run_codes = png_runs::make_codes();
__constant__ RunHeaderWords c_run_header = make_run_header_words();
__constant__ BlockOver c_run_block = make_run_block_over();
struct ClOrder { uint8_t e[png_opt::kClSymbols]; };
constexpr ClOrder make_cl_order() {
    ClOrder o{};
    for (int i = 0; i < png_opt::kClSymbols; ++i) o.e[i] = png_opt::kClOrder[i];
    return o;
}
__constant__ ClOrder c_cl_order = make_cl_order();
__constant__ CrcTable c_crc = make_crc_table();
__constant__ CrcShifts c_crc_shift = make_crc_shifts();
__constant__ CrcPowers c_crc_pow = make_crc_powers();
__constant__ CrcBlockPowers c_crc_block = make_crc_block_powers();

// the words behind the filtered stream in scratch
struct Scratch {
    uint8_t* stream;                    // n bytes, padded to whole segments
    uint4* seg;                         // per segment: table, bits, Adler A, Adler B mod 65521
    unsigned long long* start;          // per segment: the frame's bit its block begins at
    uint32_t* crc;                      // per kCrcBlock of the chunk, counted from its end: the raw remainder
    uint32_t* meta;                     // [0] the frame's byte behind the deflate data (Adler-32's place), [1] whether the frame is inside its capacity
    png_opt::OwnTable* own;             // kRunsOwn only, per segment: its own table where that is its choice
};
constexpr size_t kMetaWords = 4;
unsigned long long capacity_of(int w, int h, int variant) { return variant != kLiterals ? png_runs::frame_capacity((size_t)w, (size_t)h) : frame_capacity((size_t)w, (size_t)h); }
size_t crc_blocks(int w, int h, int variant) { return (size_t)((capacity_of(w, h, variant) + kCrcBlock - 1) / kCrcBlock); }
Scratch scratch_of(uint8_t* p, int w, int h, int variant) {
    const size_t n_seg = (size_t)segment_count((size_t)w, (size_t)h);
    Scratch s;
    s.stream = p;
    s.seg = (uint4*)(p + n_seg * kSegment);
    s.start = (unsigned long long*)(s.seg + n_seg);
    s.crc = (uint32_t*)(s.start + n_seg);
    s.meta = s.crc + crc_blocks(w, h, variant);
    s.own = (png_opt::OwnTable*)(s.meta + kMetaWords);
    return s;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// the sum of v over the workgroup's 256 threads, in every thread (part: 4 words of LDS, free again behind the call)
__device__ __forceinline__ unsigned long long group_sum(unsigned long long v, unsigned long long* part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    const unsigned long long all = part[0] + part[1] + part[2] + part[3];
    __syncthreads();
    return all;
}
// the workgroup's exclusive prefix sum of v, and the sum of all in *all
__device__ __forceinline__ uint32_t group_scan(uint32_t v, uint32_t* part, uint32_t* all) {
    const int t = threadIdx.x, lane = t & 63;
    uint32_t incl = v;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(incl, d, 64); if (lane >= d) incl += u; }
    if (lane == 63) part[t >> 6] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (int k = 0; k < (t >> 6); ++k) before += part[k];
    *all = part[0] + part[1] + part[2] + part[3];
    __syncthreads();
    return before + incl - v;
}

// Where the run that holds a thread's first byte begins and where the run that holds its last byte ends, from the threads' own breaks: `last` is 1 + the position
// of the thread's last break (0: it has none), `first` the position of its first (0xFFFFFFFF: none).  *begin: the largest `last` of the threads in front of this
// one (0 in thread 0); *end: the smallest `first` of the threads behind it.  (part: 8 words of LDS, free again behind the call)
__device__ __forceinline__ void group_run_bounds(uint32_t last, uint32_t first, uint32_t* part, uint32_t* begin, uint32_t* end) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t hi = last, lo = first;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(hi, d, 64), v = __shfl_down(lo, d, 64);
        if (lane >= d) hi = max(hi, u);
        if (lane + d < 64) lo = min(lo, v);
    }
    if (lane == 63) part[wave] = hi;
    if (lane == 0) part[4 + wave] = lo;
    __syncthreads();
    uint32_t b = __shfl_up(hi, 1, 64), e = __shfl_down(lo, 1, 64);
    if (lane == 0) b = 0;
    if (lane == 63) e = 0xFFFFFFFFu;
    for (int k = 0; k < 4; ++k) {
        if (k < wave) b = max(b, part[k]);
        if (k > wave) e = min(e, part[4 + k]);
    }
    __syncthreads();
    *begin = b; *end = e;
}

// A thread's 32 bytes of a segment of `len` bytes, at the segment's byte `at` (< len): `valid` of them lie in the segment; bit i of `brk` says that byte i begins
// a run (it differs from the byte before it, or is the segment's first), and bit `valid`, where there is one, marks the segment's end.
struct RunBytes { uint32_t word[8], brk; int valid; };
__device__ __forceinline__ RunBytes load_run_bytes(const uint8_t* __restrict__ seg, uint32_t at, uint32_t len) {
    RunBytes r;
    const uint4* src = (const uint4*)(seg + at);
    const uint4 lo = src[0], hi = src[1];
    r.word[0] = lo.x; r.word[1] = lo.y; r.word[2] = lo.z; r.word[3] = lo.w; r.word[4] = hi.x; r.word[5] = hi.y; r.word[6] = hi.z; r.word[7] = hi.w;
    r.valid = (int)(len - at < (uint32_t)kBytesPerThread ? len - at : (uint32_t)kBytesPerThread);
    uint32_t before = at ? (uint32_t)seg[at - 1] : 256u;    // (the segment's first byte differs from everything)
    r.brk = 0;
    #pragma unroll
    for (int i = 0; i < kBytesPerThread; ++i) {
        const uint32_t d = (r.word[i >> 2] >> (8 * (i & 3))) & 255u;
        r.brk |= (uint32_t)(d != before) << i;
        before = d;
    }
    if (r.valid < kBytesPerThread) r.brk = (r.brk & ((1u << r.valid) - 1u)) | 1u << r.valid;
    return r;
}
__device__ __forceinline__ uint32_t last_break(const RunBytes& r, uint32_t at) {
    const uint32_t m = r.valid < kBytesPerThread ? r.brk & ((1u << r.valid) - 1u) : r.brk;
    return m ? at + 32u - (uint32_t)__clz(m) : 0u;
}
__device__ __forceinline__ uint32_t first_break(const RunBytes& r, uint32_t at) { return r.brk ? at + (uint32_t)__ffs(r.brk) - 1u : 0xFFFFFFFFu; }

// f(symbol, extra_bits, extra) for every token that begins in the thread's bytes, in order: a literal is its byte with no extra bits, a match its length symbol
// (png_runs::match_of, with the leading bit from a count of zeros).  begin, end: group_run_bounds' of the thread's breaks; the segment's end bounds `end`.
template <typename F>
__device__ __forceinline__ void for_each_token(const RunBytes& r, uint32_t at, uint32_t len, uint32_t begin, uint32_t end, F&& f) {
    const uint32_t run_in = begin - 1u, run_out = end < len ? end : len;      // (begin >= 1 where it is read: thread 0 has its break at byte 0)
    uint32_t next = at;                                     // the place of the next token: a match moves it past what it covers
    #pragma unroll
    for (int i = 0; i < kBytesPerThread; ++i) {
        const uint32_t p = at + (uint32_t)i;
        if (i >= r.valid || p < next) continue;
        const uint32_t lo = r.brk & (0xFFFFFFFFu >> (31 - i)), hi = i < 31 ? r.brk >> (i + 1) : 0u;
        const uint32_t s = lo ? at + 31u - (uint32_t)__clz(lo) : run_in, e = hi ? p + (uint32_t)__ffs(hi) : run_out;
        const int token = png_runs::token_at((int)(e - s), (int)(p - s));
        if (token == 0) {
            f((r.word[i >> 2] >> (8 * (i & 3))) & 255u, 0u, 0u);
        } else if (token < 0) {
            next = p + (uint32_t)-token;                    // covered by a match that began in a thread in front
        } else {
            next = p + (uint32_t)token;
            const uint32_t l = (uint32_t)token - 3u;
            if (token == 258) f(285u, 0u, 0u);
            else if (l < 8u) f(257u + l, 0u, 0u);
            else { const uint32_t eb = 29u - (uint32_t)__clz(l); f(261u + 4u * eb + ((l >> eb) & 3u), eb, l & ((1u << eb) - 1u)); }
        }
    }
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
__device__ __forceinline__ uint32_t near_zero(int v) { v &= 255; return (uint32_t)min(v, 256 - v); }

__device__ __forceinline__ uint32_t dev_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    #pragma unroll 4
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = b & 1u ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
// x^(8 n_bytes) in every lane of the wave: lane k holds x^(2^(k + 3)) where bit k of n_bytes is set and 1 elsewhere; the product over the lanes
__device__ __forceinline__ uint32_t wave_x_pow_bytes(unsigned long long n_bytes) {
    const int lane = threadIdx.x & 63;
    uint32_t p = lane <= 60 && (n_bytes >> lane & 1) ? c_crc_pow.e[lane + 3] : 1u << 31;
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) p = dev_crc_mul(p, __shfl_xor(p, d, 64));
    return p;
}

}  // namespace

namespace {

// byte k of four consecutive dwords
__device__ __forceinline__ int byte_of(const uint32_t (&d)[4], int k) { return (int)((d[k >> 2] >> (8 * (k & 3))) & 255u); }

// f(cur, a, b, c, at) for every byte of row y that the thread takes: the byte, its neighbours left, above and above left (zeros outside the frame) and the byte's
// place among the row's 3 w filtered bytes (B, G, R -> R, G, B).  WIDE (w a multiple of 4, the frame 4-byte aligned, so every row is): four pixels per trip from
// three dwords of either row and the dword in front of them, whose upper three bytes are the pixel to the left; else a pixel per trip, bytewise.
template <bool WIDE, typename F>
__device__ __forceinline__ void for_each_byte(const uint8_t* __restrict__ row, const uint8_t* __restrict__ above, int w, int y, F&& f) {
    if (WIDE) {
        const uint32_t *r32 = (const uint32_t*)row, *a32 = (const uint32_t*)above;
        for (int q = threadIdx.x; q < w / 4; q += kThreads) {
            const size_t at = 3 * (size_t)q;
            const uint32_t cw[4] = {q ? r32[at - 1] : 0u, r32[at], r32[at + 1], r32[at + 2]};
            const uint32_t aw[4] = {q && y ? a32[at - 1] : 0u, y ? a32[at] : 0u, y ? a32[at + 1] : 0u, y ? a32[at + 2] : 0u};
            #pragma unroll
            for (int i = 0; i < 12; ++i) f(byte_of(cw, 4 + i), byte_of(cw, 1 + i), byte_of(aw, 4 + i), byte_of(aw, 1 + i), 4 * at + (size_t)(3 * (i / 3) + 2 - i % 3));
        }
    } else {
        for (int x = threadIdx.x; x < w; x += kThreads) {
            #pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const size_t at = 3 * (size_t)x + ch;
                f((int)row[at], x ? (int)row[at - 3] : 0, y ? (int)above[at] : 0, x && y ? (int)above[at - 3] : 0, 3 * (size_t)x + (size_t)(2 - ch));
            }
        }
    }
}

}  // namespace

template <bool WIDE>
__global__ void __launch_bounds__(kThreads) k_png_filter(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ stream, int w) {
    __shared__ unsigned long long s_part[5][4];
    __shared__ int s_type;
    const int t = threadIdx.x, y = blockIdx.x;
    const size_t row_bytes = 3 * (size_t)w;
    const uint8_t *row = bgr + (size_t)y * row_bytes, *above = row - row_bytes;      // (`above` is read in rows 1.. only)
    uint32_t score[5] = {0, 0, 0, 0, 0};
    for_each_byte<WIDE>(row, above, w, y, [&](int cur, int a, int b, int c, size_t) {
        score[0] += near_zero(cur); score[1] += near_zero(cur - a); score[2] += near_zero(cur - b);
        score[3] += near_zero(cur - ((a + b) >> 1)); score[4] += near_zero(cur - paeth(a, b, c));
    });
    #pragma unroll
    for (int k = 0; k < 5; ++k) {
        const unsigned long long v = wave_sum(score[k]);
        if ((t & 63) == 0) s_part[k][t >> 6] = v;
    }
    __syncthreads();
    if (t == 0) {
        int best = 0; unsigned long long least = 0;
        for (int k = 0; k < 5; ++k) {
            const unsigned long long v = s_part[k][0] + s_part[k][1] + s_part[k][2] + s_part[k][3];
            if (k == 0 || v < least) { best = k; least = v; }
        }
        s_type = best;
    }
    __syncthreads();
    const int type = s_type;
    uint8_t* out = stream + (size_t)y * (1 + row_bytes);
    if (t == 0) out[0] = (uint8_t)type;
    for_each_byte<WIDE>(row, above, w, y, [&](int cur, int a, int b, int c, size_t at) {
        const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
        out[1 + at] = (uint8_t)(cur - pred);
    });
}

__global__ void __launch_bounds__(kThreads) k_png_cost(const uint8_t* __restrict__ stream, uint4* __restrict__ seg_info, unsigned long long n) {
    __shared__ uint32_t s_nib[256];
    __shared__ unsigned long long s_part[4];
    const int t = threadIdx.x;
    const size_t first = (size_t)blockIdx.x * kSegment;
    const uint32_t len = (uint32_t)(n - first < kSegment ? n - first : kSegment);
    s_nib[t] = c_nibbles.e[t];
    __syncthreads();
    uint32_t cost[kTables] = {0, 0, 0, 0, 0, 0, 0, 0}, sum = 0, weighted = 0;
    const uint32_t at = (uint32_t)t * kBytesPerThread;
    if (at < len) {
        const uint4* src = (const uint4*)(stream + first + at);
        const uint4 lo = src[0], hi = src[1];
        const uint32_t word[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        #pragma unroll
        for (int i = 0; i < kBytesPerThread; ++i) {
            if (at + i >= len) break;
            const uint32_t d = (word[i >> 2] >> (8 * (i & 3))) & 255u, v = s_nib[d];
            #pragma unroll
            for (int k = 0; k < kTables; ++k) cost[k] += (v >> (4 * k)) & 15u;
            sum += d; weighted += (len - (at + i)) * d;      // (at most 32 * 8192 * 255: no overflow)
        }
    }
    unsigned long long total[kTables];
    #pragma unroll
    for (int k = 0; k < kTables; ++k) total[k] = group_sum(cost[k], s_part);
    const unsigned long long a = group_sum(sum, s_part), b = group_sum(weighted % kAdlerMod, s_part);
    if (t == 0) {
        int best = 0; unsigned long long least = 0;
        for (int k = 0; k < kTables; ++k) {
            const unsigned long long v = total[k] + c_block.over[k];
            if (k == 0 || v < least) { best = k; least = v; }
        }
        seg_info[blockIdx.x] = make_uint4((uint32_t)best, (uint32_t)least, (uint32_t)a, (uint32_t)(b % kAdlerMod));
    }
}

__global__ void __launch_bounds__(kThreads) k_png_scan(const uint4* __restrict__ seg_info, unsigned long long* __restrict__ seg_start, uint32_t* __restrict__ meta,
                                                       uint32_t* __restrict__ frame32, uint32_t n_seg, unsigned long long n, uint32_t w, uint32_t h,
                                                       uint32_t ihdr_crc, unsigned long long capacity) {
    __shared__ uint32_t s_part[4];
    __shared__ unsigned long long s_sum[4];
    __shared__ uint32_t s_head[12];
    const uint32_t t = threadIdx.x;
    const unsigned long long cap_words = (capacity + 3) / 4;
    unsigned long long at = kFirstBit, adler_a = 0, adler_b = 0;
    for (uint32_t base = 0; base < n_seg; base += kThreads) {
        const uint32_t i = base + t;
        const bool valid = i < n_seg;
        const uint4 info = valid ? seg_info[i] : make_uint4(0, 0, 0, 0);
        uint32_t all = 0;
        const uint32_t before = group_scan(info.y, s_part, &all);
        if (valid) {
            const unsigned long long start = at + before, first = (unsigned long long)i * kSegment, len = n - first < kSegment ? n - first : kSegment;
            seg_start[i] = start;
            if (i && (start >> 5) < cap_words) frame32[start >> 5] = 0;      // the word this block shares with the one before it
            adler_a += info.z;
            adler_b = (adler_b + ((n - first - len) % kAdlerMod) * (info.z % kAdlerMod) + info.w) % kAdlerMod;
        }
        at += all;
    }
    adler_a = group_sum(adler_a, s_sum);
    adler_b = group_sum(adler_b, s_sum);
    if (t != 0) return;
    const unsigned long long end = (at + 7) >> 3, total = end + kTailBytes;      // `end`: the frame's byte behind the deflate data
    const bool ok = total <= capacity && total < (1ull << 31);
    meta[0] = (uint32_t)end; meta[1] = ok;
    if (!ok) { frame32[0] = 0; return; }
    const uint32_t a = (uint32_t)((1 + adler_a) % kAdlerMod), b = (uint32_t)((n % kAdlerMod + adler_b) % kAdlerMod);
    uint8_t *head = (uint8_t*)s_head, *frame = (uint8_t*)frame32;
    auto be32 = [](uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; };
    s_head[0] = (uint32_t)total;
    for (int k = 0; k < 8; ++k) head[kOffSignature + k] = c_fixed.signature[k];
    be32(head + kOffIhdr, 13);
    head[kOffIhdr + 4] = 'I'; head[kOffIhdr + 5] = 'H'; head[kOffIhdr + 6] = 'D'; head[kOffIhdr + 7] = 'R';
    be32(head + kOffIhdr + 8, w); be32(head + kOffIhdr + 12, h);
    head[kOffIhdr + 16] = 8; head[kOffIhdr + 17] = 2; head[kOffIhdr + 18] = 0; head[kOffIhdr + 19] = 0; head[kOffIhdr + 20] = 0;
    be32(head + kOffIhdr + 21, ihdr_crc);
    be32(head + kOffIdat, (uint32_t)(end + 4 - (kOffIdatType + 4)));
    head[kOffIdatType] = 'I'; head[kOffIdatType + 1] = 'D'; head[kOffIdatType + 2] = 'A'; head[kOffIdatType + 3] = 'T';
    head[kOffIdatType + 4] = 0x78; head[kOffIdatType + 5] = 0x01;
    head[kStreamByte] = 0;                                  // the first block's bits are ORed into this word
    static_assert(kStreamByte == 47 && sizeof s_head == 48, "the head is twelve whole words");
    for (int k = 0; k < 12; ++k) frame32[k] = s_head[k];
    frame32[at >> 5] = 0;                                   // the word the stream ends in: the last block ORs its bits into it, the bytes below follow them
    be32(frame + end, b << 16 | a);
    for (int k = 0; k < 12; ++k) frame[end + 8 + k] = c_fixed.iend[k];
}

__global__ void __launch_bounds__(kThreads) k_png_pack(const uint8_t* __restrict__ stream, const uint4* __restrict__ seg_info, const unsigned long long* __restrict__ seg_start,
                                                       const uint32_t* __restrict__ meta, uint32_t* __restrict__ frame32, uint32_t n_seg, unsigned long long n,
                                                       unsigned long long capacity) {
    __shared__ uint32_t s_image[kImageWords];
    __shared__ uint32_t s_code[kSymbols];
    __shared__ uint32_t s_part[4];
    const int t = threadIdx.x;
    const uint32_t seg = blockIdx.x;
    const uint4 info = seg_info[seg];
    const uint32_t table = info.x & (kTables - 1), bits = info.y;
    if (!meta[1] || bits > kSegmentBitsMax) return;         // (never: the scan found the frame inside its capacity, and table 7 bounds every block)
    const unsigned long long start = seg_start[seg];
    const size_t first = (size_t)seg * kSegment;
    const uint32_t len = (uint32_t)(n - first < kSegment ? n - first : kSegment);
    const uint32_t off = (uint32_t)start & 31u, n_words = (off + bits + 31) >> 5;
    for (uint32_t i = t; i < n_words; i += kThreads) s_image[i] = 0;
    for (int i = t; i < kSymbols; i += kThreads) s_code[i] = c_codes.e[table][i];
    __syncthreads();
    const uint32_t header_bits = c_block.header[table];
    for (uint32_t i = t; 32 * i < header_bits; i += kThreads) {      // the header, a word per thread (the bits behind H_k are zeros in the table)
        const uint32_t v = c_header.e[table][i] | (i == 0 && seg == n_seg - 1 ? 1u : 0u), p = off + 32 * i;
        atomicOr(&s_image[p >> 5], v << (p & 31));
        if ((p & 31) && (v >> (32 - (p & 31)))) atomicOr(&s_image[(p >> 5) + 1], v >> (32 - (p & 31)));
    }
    const uint32_t at = (uint32_t)t * kBytesPerThread;
    uint32_t word[8] = {0, 0, 0, 0, 0, 0, 0, 0}, count = 0;
    if (at < len) {
        const uint4* src = (const uint4*)(stream + first + at);
        const uint4 lo = src[0], hi = src[1];
        word[0] = lo.x; word[1] = lo.y; word[2] = lo.z; word[3] = lo.w; word[4] = hi.x; word[5] = hi.y; word[6] = hi.z; word[7] = hi.w;
        #pragma unroll
        for (int i = 0; i < kBytesPerThread; ++i)
            if (at + i < len) count += s_code[(word[i >> 2] >> (8 * (i & 3))) & 255u] & 15u;
    }
    uint32_t all = 0;
    const uint32_t before = group_scan(count, s_part, &all);
    if (at < len) {
        const uint32_t p = off + header_bits + before;
        uint32_t at_word = p >> 5;
        int n_acc = (int)(p & 31);
        unsigned long long acc = 0;
        auto put = [&](uint32_t e) {                        // a code of at most 15 bits behind fewer than 32 waiting ones
            acc |= (unsigned long long)(e >> 4) << n_acc;
            n_acc += (int)(e & 15u);
            if (n_acc >= 32) { atomicOr(&s_image[at_word++], (uint32_t)acc); acc >>= 32; n_acc -= 32; }
        };
        #pragma unroll
        for (int i = 0; i < kBytesPerThread; ++i)
            if (at + i < len) put(s_code[(word[i >> 2] >> (8 * (i & 3))) & 255u]);
        if (at + kBytesPerThread >= len) put(s_code[kEob]);      // the thread of the segment's last byte: end-of-block
        if (n_acc) atomicOr(&s_image[at_word], (uint32_t)acc);
    }
    __syncthreads();
    const unsigned long long word0 = start >> 5, word_end = (start + bits) >> 5, cap_words = (capacity + 3) / 4;
    for (uint32_t i = t; i < n_words; i += kThreads) {
        const unsigned long long fw = word0 + i;
        if (fw >= cap_words) continue;
        if (fw == word0 || fw == word_end) atomicOr(&frame32[fw], s_image[i]); else frame32[fw] = s_image[i];
    }
}

namespace {

// k_png_run_cost's body.  SEQ (k_png_seq_cost): a ninth candidate, the sequence's table, whose lengths (its entries' low nibbles) stand in LDS beside the eight
// fixed tables' nibbles; its cost is its header, the tokens' codes, the same extra and distance bits and its end-of-block code.  Ties go to the fixed tables.
template <bool SEQ>
__device__ __forceinline__ void run_cost(const uint8_t* __restrict__ stream, uint4* __restrict__ seg_info, const png_opt::OwnTable* __restrict__ shared, unsigned long long n) {
    __shared__ uint32_t s_nib[png_runs::kSymbols];
    __shared__ uint32_t s_ninth[SEQ ? png_runs::kSymbols : 1];
    __shared__ unsigned long long s_part[4];
    __shared__ uint32_t s_bound[8];
    const int t = threadIdx.x;
    const size_t first = (size_t)blockIdx.x * kSegment;
    const uint32_t len = (uint32_t)(n - first < kSegment ? n - first : kSegment);
    for (int i = t; i < png_runs::kSymbols; i += kThreads) { s_nib[i] = c_run_nibbles.e[i]; if (SEQ) s_ninth[i] = shared->code[i] & 15u; }
    uint32_t cost[kTables] = {0, 0, 0, 0, 0, 0, 0, 0}, ninth = 0, beside = 0, sum = 0, weighted = 0;
    const uint32_t at = (uint32_t)t * kBytesPerThread;
    const bool active = at < len;
    RunBytes r{};
    if (active) r = load_run_bytes(stream + first, at, len);
    uint32_t begin = 0, end = 0;
    group_run_bounds(active ? last_break(r, at) : 0u, active ? first_break(r, at) : 0xFFFFFFFFu, s_bound, &begin, &end);      // (its barrier stands behind s_nib's stores too)
    if (active) {
        for_each_token(r, at, len, begin, end, [&](uint32_t symbol, uint32_t extra_bits, uint32_t) {
            const uint32_t v = s_nib[symbol];
            #pragma unroll
            for (int k = 0; k < kTables; ++k) cost[k] += (v >> (4 * k)) & 15u;
            if (SEQ) ninth += s_ninth[symbol];
            if (symbol > (uint32_t)kEob) beside += extra_bits + 1u;      // a match's extra bits and its distance code, whatever the table
        });
        #pragma unroll
        for (int i = 0; i < kBytesPerThread; ++i) {
            const uint32_t d = i < r.valid ? (r.word[i >> 2] >> (8 * (i & 3))) & 255u : 0u;
            sum += d; weighted += (len - (at + i)) * d;      // (at most 32 * 8192 * 255: no overflow)
        }
    }
    unsigned long long total[kTables];
    #pragma unroll
    for (int k = 0; k < kTables; ++k) total[k] = group_sum(cost[k] + beside, s_part);
    const unsigned long long a = group_sum(sum, s_part), b = group_sum(weighted % kAdlerMod, s_part);
    const unsigned long long ninth_all = SEQ ? group_sum(ninth + beside, s_part) : 0ull;
    if (t == 0) {
        int best = 0; unsigned long long least = 0;
        for (int k = 0; k < kTables; ++k) {
            const unsigned long long v = total[k] + c_run_block.over[k];
            if (k == 0 || v < least) { best = k; least = v; }
        }
        if (SEQ) {
            const unsigned long long v = ninth_all + shared->header_bits + s_ninth[kEob];
            if (v < least) { best = png_opt::kOwn; least = v; }
        }
        seg_info[blockIdx.x] = make_uint4((uint32_t)best, (uint32_t)least, (uint32_t)a, (uint32_t)(b % kAdlerMod));
    }
}

}  // namespace

__global__ void __launch_bounds__(kThreads) k_png_run_cost(const uint8_t* __restrict__ stream, uint4* __restrict__ seg_info, unsigned long long n) {
    run_cost<false>(stream, seg_info, nullptr, n);
}

// POPPY_FRAME_PNG_SEQ's choice, behind the sequence's build: k_png_run_cost with the sequence's table as the ninth candidate
__global__ void __launch_bounds__(kThreads) k_png_seq_cost(const uint8_t* __restrict__ stream, uint4* __restrict__ seg_info, const png_opt::OwnTable* __restrict__ shared, unsigned long long n) {
    run_cost<true>(stream, seg_info, shared, n);
}

namespace {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

constexpr int kLanes = 64, kPerLane = 5;                    // a lane holds symbols (and places of the header's sequence) lane + 64 j
static_assert(kLanes * kPerLane >= png_opt::kSequenceMax + 1, "five per lane cover the 286 symbols, and the 287 places of the sequence with the mark behind them");
struct BuildLds {
    uint32_t of_depth[png_opt::kSymbols + 2];               // the symbols of each depth 0..286, then of each length
    uint32_t key[png_opt::kSymbols];                        // a symbol's (depth, then length) << 9 | symbol, ~0 without a code
    uint32_t first_code[16], first_place[16];               // per length: its first canonical code, the place of its first symbol
};
constexpr unsigned long long kNoKey = ~0ull;

// a symbol's place among the n keys: the number of smaller ones
__device__ __forceinline__ void places_of(const uint32_t* key, int n, int lane, uint32_t (&place)[kPerLane]) {
    uint32_t mine[kPerLane];
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) { const int idx = lane + kLanes * j; mine[j] = idx < n ? key[idx] : ~0u; place[j] = 0; }
    for (int i = 0; i < n; ++i) {
        const uint32_t other = key[i];
        #pragma unroll
        for (int j = 0; j < kPerLane; ++j) place[j] += other < mine[j];
    }
}

// The two smallest of the wave's keys (unique, or kNoKey) in every lane, from every lane's own two smallest: a butterfly over the lanes in which the pairs (a1, a2)
// and (b1, b2) merge into (min(a1, b1), min(max(a1, b1), min(a2, b2))).  Twelve 64-bit shuffles and no LDS word: written as atomicMin on an LDS word, the
// compiler makes each of the two minima a scalar loop over the active lanes, and reading the word back is a flat load — 5 us per merge where this takes a tenth.
__device__ __forceinline__ void wave_two_smallest(unsigned long long& m1, unsigned long long& m2) {
    #pragma unroll
    for (int d = 1; d < kLanes; d <<= 1) {
        const unsigned long long o1 = __shfl_xor(m1, d, kLanes), o2 = __shfl_xor(m2, d, kLanes);
        const unsigned long long lo = m1 < o1 ? m1 : o1, hi = m1 < o1 ? o1 : m1, rest = m2 < o2 ? m2 : o2;
        m1 = lo; m2 = hi < rest ? hi : rest;
    }
}

// poppy_png_optimal_lengths' rule (include/poppy_hip.h) in one wave, every lane of which is here: freq[j] is the count of symbol lane + 64 j (0 from n on, and at
// least one is not), n <= 286, the used symbols no more than 2^limit.  entry[j]: the symbol's reversed canonical code << 4 | its length, 0 without a code.
__device__ __forceinline__ void build_code(uint32_t (&freq)[kPerLane], int n, int limit, BuildLds& L, uint32_t (&entry)[kPerLane]) {
    const int lane = threadIdx.x & (kLanes - 1);
    int tree[kPerLane], depth[kPerLane];
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) { tree[j] = lane + kLanes * j; depth[j] = 0; }
    for (int i = lane; i < png_opt::kSymbols + 2; i += kLanes) L.of_depth[i] = 0;
    bool merged = false;
    unsigned long long m1, m2;
    for (;;) {
        // the two smallest keys of the wave (keys are unique): the lane's own pair, then the butterfly
        m1 = kNoKey; m2 = kNoKey;
        #pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            const unsigned long long key = freq[j] ? (unsigned long long)freq[j] << 9 | (unsigned long long)(511 - (lane + kLanes * j)) : kNoKey;
            if (key < m1) { m2 = m1; m1 = key; } else if (key < m2) m2 = key;
        }
        wave_two_smallest(m1, m2);
        if (m2 == kNoKey) break;                            // (wave-uniform: every lane holds the same pair)
        merged = true;
        const int c1 = 511 - (int)(m1 & 511), c2 = 511 - (int)(m2 & 511);
        const uint32_t f2 = (uint32_t)(m2 >> 9);
        #pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            const int idx = lane + kLanes * j;
            if (tree[j] == c1 || tree[j] == c2) { ++depth[j]; tree[j] = c1; }
            if (idx == c1) freq[j] += f2;
            if (idx == c2) freq[j] = 0;
        }
    }
    wave_sync();                                            // (of_depth's zeros stand before other lanes count into them)
    int longest = 0;
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const int idx = lane + kLanes * j;
        if (!merged && m1 != kNoKey && idx == 511 - (int)(m1 & 511)) depth[j] = 1;      // a single symbol with a count
        if (depth[j]) atomicAdd(&L.of_depth[depth[j]], 1u);
        longest = max(longest, depth[j]);
        if (idx < n) L.key[idx] = depth[j] ? (uint32_t)depth[j] << 9 | (uint32_t)idx : ~0u;
    }
    #pragma unroll
    for (int d = 1; d < kLanes; d <<= 1) longest = max(longest, __shfl_xor(longest, d, kLanes));
    wave_sync();
    if (lane == 0) {
        uint32_t* bits = L.of_depth;
        for (int i = longest; i > limit; --i)               // Annex K.3
            while (bits[i] > 0) {
                int j = i - 2;
                while (j > 0 && bits[j] == 0) --j;
                bits[i] -= 2; bits[i - 1] += 1; bits[j + 1] += 2; bits[j] -= 1;
            }
        uint32_t code = 0, place = 0;
        for (int l = 1; l <= 15; ++l) {
            L.first_code[l] = code; L.first_place[l] = place;
            code = (code + bits[l]) << 1; place += bits[l];
        }
    }
    wave_sync();
    // by depth, then by symbol, the adjusted lengths in ascending order: the length whose places hold the symbol's
    uint32_t place[kPerLane], length[kPerLane];
    places_of(L.key, n, lane, place);
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        length[j] = 0;
        if (depth[j])
            for (int l = 1; l <= 15; ++l)
                if (place[j] >= L.first_place[l] && place[j] - L.first_place[l] < L.of_depth[l]) length[j] = (uint32_t)l;
    }
    wave_sync();
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) { const int idx = lane + kLanes * j; if (idx < n) L.key[idx] = length[j] ? length[j] << 9 | (uint32_t)idx : ~0u; }
    wave_sync();
    // deflate's canonical code: by length, then by symbol
    places_of(L.key, n, lane, place);
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const uint32_t l = length[j], code = l ? L.first_code[l] + place[j] - L.first_place[l] : 0u;
        entry[j] = l ? (__brev(code) >> (32 - l)) << 4 | l : 0u;
    }
    wave_sync();                                            // (L is free again)
}

// `width` bits (at most 32) of `value` into a bit string in LDS, at its bit `at`
__device__ __forceinline__ void or_bits(uint32_t* words, uint32_t at, uint32_t value, uint32_t width) {
    if (!width) return;
    const unsigned long long v = (unsigned long long)value << (at & 31);
    atomicOr(&words[at >> 5], (uint32_t)v);
    if ((at & 31) + width > 32) atomicOr(&words[(at >> 5) + 1], (uint32_t)(v >> 32));
}

// What place lane + 64 j of the header's length sequence `seq` (n_seq places) sends: brk holds the sequence's breaks, bit p of the five words together set where place
// p begins a run, and at p = n_seq.  The run's first place is the last break at or before p (place 0 is one), its end the first break behind p; png_opt::entry_at
// decides from them.  -1: nothing (a place that an earlier entry covers, or none of the sequence); else symbol | extra bits << 8 | extra value << 16.
__device__ __forceinline__ int sent_at(const unsigned long long (&brk)[kPerLane], int j, int lane, int n_seq, const uint32_t* seq) {
    const int p = lane + kLanes * j;
    int start = 0, stop = n_seq;
    #pragma unroll
    for (int w = 0; w < kPerLane; ++w) {
        const unsigned long long m = w < j ? brk[w] : w == j ? brk[w] & (~0ull >> (63 - lane)) : 0ull;
        if (m) start = kLanes * w + 63 - __clzll((long long)m);
    }
    #pragma unroll
    for (int w = kPerLane - 1; w >= 0; --w) {
        const unsigned long long m = w > j ? brk[w] : w == j && lane < 63 ? brk[w] & (~0ull << (lane + 1)) : 0ull;
        if (m) stop = kLanes * w + __ffsll((long long)m) - 1;
    }
    if (p >= n_seq) return -1;
    const png_opt::Entry e = png_opt::entry_at((int)seq[start], stop - start, p - start);
    return e.symbol < 0 ? -1 : e.symbol | e.extra_bits << 8 | (int)(e.extra << 16);
}

// What the own header of a table needs in LDS: the length sequence, the code-length symbols' counts and then their entries, the header's bits
struct HeaderLds { uint32_t seq[kLanes * kPerLane], cl[32], header[png_opt::kOwnHeaderWords + 1]; };

// The own header of a table (include/poppy_hip.h: Block header) in one wave, every lane of which is here: entry[j] is build_code's of symbol lane + 64 j.  The
// lanes' break flags are five ballots, so every place of the length sequence finds its run by itself (sent_at); the 19 counts, the same build at 7 bits, a prefix
// sum of the entries' bits, and the header ORed into H.header, BFINAL 0, zeros behind it.  Returns the header's bits.
__device__ __forceinline__ uint32_t own_header(const uint32_t (&entry)[kPerLane], HeaderLds& H, BuildLds& L) {
    const int lane = threadIdx.x & (kLanes - 1);
    uint32_t* const s_seq = H.seq; uint32_t* const s_cl = H.cl; uint32_t* const s_header = H.header;
    int n_lit = 257;
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) if (entry[j]) n_lit = max(n_lit, lane + kLanes * j + 1);
    #pragma unroll
    for (int d = 1; d < kLanes; d <<= 1) n_lit = max(n_lit, __shfl_xor(n_lit, d, kLanes));
    // the length sequence: the lit/len lengths, then the distance code's 1; place n_seq carries the mark that ends the last run
    const int n_seq = n_lit + 1;
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) { const int p = lane + kLanes * j; s_seq[p] = p < n_lit ? entry[j] & 15u : 1u; }
    if (lane < 32) s_cl[lane] = 0;
    for (int i = lane; i < png_opt::kOwnHeaderWords + 1; i += kLanes) s_header[i] = 0;
    wave_sync();
    unsigned long long brk[kPerLane];
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const int p = lane + kLanes * j;
        brk[j] = __ballot(p < n_seq ? p == 0 || s_seq[p] != s_seq[p - 1] : p == n_seq);
    }
    int sent[kPerLane];                                     // what a place sends: the code-length symbol, its extra bits << 8 and their value << 16; -1 for nothing
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        sent[j] = sent_at(brk, j, lane, n_seq, s_seq);
        if (sent[j] >= 0) atomicAdd(&s_cl[sent[j] & 31], 1u);
    }
    wave_sync();
    uint32_t cl_freq[kPerLane] = {lane < png_opt::kClSymbols ? s_cl[lane] : 0u, 0u, 0u, 0u, 0u}, cl_entry[kPerLane];
    build_code(cl_freq, png_opt::kClSymbols, png_opt::kClLimit, L, cl_entry);
    if (lane < png_opt::kClSymbols) s_cl[lane] = cl_entry[0];
    wave_sync();
    // HCLEN: the code-length code's lengths in RFC 1951's order, trailing zeros trimmed, at least 4
    const uint32_t ordered = lane < png_opt::kClSymbols ? s_cl[c_cl_order.e[lane]] & 15u : 0u;
    const unsigned long long has = __ballot(ordered != 0);
    const int n_cl = max(4, has ? 64 - __clzll((long long)has) : 0);
    uint32_t at_bit = 17u + 3u * (uint32_t)n_cl;
    if (lane == 0) or_bits(s_header, 0, 4u | (uint32_t)(n_lit - 257) << 3 | (uint32_t)(n_cl - 4) << 13, 17);      // BFINAL 0, BTYPE 10, HLIT, HDIST 0, HCLEN
    if (lane < n_cl) or_bits(s_header, 17u + 3u * (uint32_t)lane, ordered, 3);
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) {                    // the entries' places in the header: a prefix sum of their bits in the sequence's order
        const uint32_t e = sent[j] >= 0 ? s_cl[sent[j] & 31] : 0u, code_bits = e & 15u, width = sent[j] >= 0 ? code_bits + ((uint32_t)sent[j] >> 8 & 15u) : 0u;
        uint32_t incl = width;
        #pragma unroll
        for (int d = 1; d < kLanes; d <<= 1) { const uint32_t u = __shfl_up(incl, d, kLanes); if (lane >= d) incl += u; }
        or_bits(s_header, at_bit + incl - width, e >> 4 | ((uint32_t)sent[j] >> 16) << code_bits, width);      // the code, then the extra bits: 7 + 7 at the most
        at_bit += __shfl(incl, kLanes - 1, kLanes);
    }
    wave_sync();
    return at_bit;
}

// A segment of `len` bytes by its workgroup: its tokens counted into the histogram s_count (kLanes * kPerLane words; end-of-block counts 1, zeros behind 285), with a
// barrier behind the last ds_add.  The thread's own share of what no table changes comes back: the extra and distance bits of the matches that begin in its
// bytes, and its bytes' sums for the Adler pair.  (s_bound: group_run_bounds' 8 words)
struct SegmentSums { uint32_t beside, sum, weighted; };
__device__ __forceinline__ SegmentSums count_tokens(const uint8_t* __restrict__ seg, uint32_t len, uint32_t* s_count, uint32_t* s_bound) {
    const int t = threadIdx.x;
    for (int i = t; i < kLanes * kPerLane; i += kThreads) s_count[i] = i == kEob ? 1u : 0u;
    uint32_t beside = 0, sum = 0, weighted = 0;
    const uint32_t at = (uint32_t)t * kBytesPerThread;
    const bool active = at < len;
    RunBytes r{};
    if (active) r = load_run_bytes(seg, at, len);
    uint32_t begin = 0, end = 0;
    group_run_bounds(active ? last_break(r, at) : 0u, active ? first_break(r, at) : 0xFFFFFFFFu, s_bound, &begin, &end);      // (its barrier stands behind s_count's stores too)
    if (active) {
        for_each_token(r, at, len, begin, end, [&](uint32_t symbol, uint32_t extra_bits, uint32_t) {
            atomicAdd(&s_count[symbol], 1u);
            if (symbol > (uint32_t)kEob) beside += extra_bits + 1u;      // a match's extra bits and its distance code, whatever the table
        });
        #pragma unroll
        for (int i = 0; i < kBytesPerThread; ++i) {
            const uint32_t d = i < r.valid ? (r.word[i >> 2] >> (8 * (i & 3))) & 255u : 0u;
            sum += d; weighted += (len - (at + i)) * d;      // (at most 32 * 8192 * 255: no overflow)
        }
    }
    __syncthreads();
    return SegmentSums{beside, sum, weighted};
}

// a built table into its record: the symbols' entries, the header's bits and their number (one wave)
__device__ __forceinline__ void store_table(png_opt::OwnTable* __restrict__ own, const uint32_t (&entry)[kPerLane], uint32_t at_bit, const HeaderLds& H) {
    const int lane = threadIdx.x & (kLanes - 1);
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) { const int idx = lane + kLanes * j; if (idx < png_opt::kSymbols) own->code[idx] = entry[j]; }
    if (lane == 0) own->header_bits = at_bit;
    for (int i = lane; i < png_opt::kOwnHeaderWords + 1; i += kLanes) own->header[i] = H.header[i];
}

}  // namespace

__global__ void __launch_bounds__(kThreads) k_png_opt_cost(const uint8_t* __restrict__ stream, uint4* __restrict__ seg_info, png_opt::OwnTable* __restrict__ own, unsigned long long n) {
    __shared__ uint32_t s_count[kLanes * kPerLane];         // the tokens of each symbol; zeros behind 285
    __shared__ HeaderLds s_head;                            // the own header in the making
    __shared__ BuildLds s_build;
    __shared__ unsigned long long s_part[4];
    __shared__ uint32_t s_bound[8];
    const int t = threadIdx.x;
    const size_t first = (size_t)blockIdx.x * kSegment;
    const uint32_t len = (uint32_t)(n - first < kSegment ? n - first : kSegment);
    const SegmentSums mine = count_tokens(stream + first, len, s_count, s_bound);
    const uint32_t beside = mine.beside, sum = mine.sum, weighted = mine.weighted;
    uint32_t cost[kTables] = {0, 0, 0, 0, 0, 0, 0, 0};      // the fixed tables: the histogram's dot products with their lengths (end-of-block is in it)
    for (int i = t; i < png_runs::kSymbols; i += kThreads) {
        const uint32_t c = s_count[i], v = c_run_nibbles.e[i];
        #pragma unroll
        for (int k = 0; k < kTables; ++k) cost[k] += c * ((v >> (4 * k)) & 15u);
    }
    unsigned long long total[kTables];
    #pragma unroll
    for (int k = 0; k < kTables; ++k) total[k] = group_sum(cost[k] + beside, s_part);
    const unsigned long long a = group_sum(sum, s_part), b = group_sum(weighted % kAdlerMod, s_part), beside_all = group_sum(beside, s_part);
    if (t >= kLanes) return;                                // wave 0 builds the own table: no workgroup barrier from here on
    int best = 0; unsigned long long least = 0;
    for (int k = 0; k < kTables; ++k) {
        const unsigned long long v = total[k] + c_run_block.header[k];
        if (k == 0 || v < least) { best = k; least = v; }
    }
    const int lane = t;
    uint32_t freq[kPerLane], count[kPerLane], entry[kPerLane];
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) count[j] = freq[j] = s_count[lane + kLanes * j];
    build_code(freq, png_opt::kSymbols, png_opt::kLimit, s_build, entry);
    unsigned long long own_bits = 0;
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) own_bits += (unsigned long long)count[j] * (entry[j] & 15u);
    own_bits = wave_sum(own_bits);
    const uint32_t at_bit = own_header(entry, s_head, s_build);
    const unsigned long long own_cost = (unsigned long long)at_bit + own_bits + beside_all;
    const bool owned = own_cost < least;                    // (ties go to the lowest index: a fixed table)
    if (lane == 0) seg_info[blockIdx.x] = make_uint4(owned ? (uint32_t)png_opt::kOwn : (uint32_t)best, (uint32_t)(owned ? own_cost : least), (uint32_t)a, (uint32_t)(b % kAdlerMod));
    if (!owned) return;
    store_table(own + blockIdx.x, entry, at_bit, s_head);
}

// POPPY_FRAME_PNG_SEQ's counting pass, a workgroup per segment of a frame that has just been filtered into its place in the sequence store: k_png_opt_cost's
// histogram, then its non-zero words added to the sequence's 286 sums (end-of-block: 1 per segment).  No sum passes 2^32 - 1: png_seq_fits.
__global__ void __launch_bounds__(kThreads) k_png_seq_count(const uint8_t* __restrict__ stream, uint32_t* __restrict__ sums, unsigned long long n) {
    __shared__ uint32_t s_count[kLanes * kPerLane];
    __shared__ uint32_t s_bound[8];
    const size_t first = (size_t)blockIdx.x * kSegment;
    const uint32_t len = (uint32_t)(n - first < kSegment ? n - first : kSegment);
    (void)count_tokens(stream + first, len, s_count, s_bound);
    for (int i = threadIdx.x; i < png_runs::kSymbols; i += kThreads) if (s_count[i]) atomicAdd(&sums[i], s_count[i]);
}

// POPPY_FRAME_PNG_SEQ's one build per sequence, one wave: the sums (zero again behind it) -> the sequence's table, as k_png_opt_cost's wave 0 builds a segment's:
// build_code at 15 bits, then the own header.  The counts here are a whole sequence's, up to 2^32 - 1 in all: build_code's keys are count << 9 | 511 - symbol in
// 64 bits, a merged count is a sum of counts and so below 2^32 too, the depths are counted per symbol (286 at the most), and nothing here multiplies a count.
__global__ void __launch_bounds__(kLanes) k_png_seq_table(uint32_t* __restrict__ sums, png_opt::OwnTable* __restrict__ table) {
    __shared__ HeaderLds s_head;
    __shared__ BuildLds s_build;
    const int lane = threadIdx.x;
    uint32_t freq[kPerLane], entry[kPerLane];
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const int idx = lane + kLanes * j;
        freq[j] = idx < png_opt::kSymbols ? sums[idx] : 0u;
        if (idx < png_opt::kSymbols) sums[idx] = 0;
    }
    build_code(freq, png_opt::kSymbols, png_opt::kLimit, s_build, entry);
    const uint32_t at_bit = own_header(entry, s_head, s_build);
    store_table(table, entry, at_bit, s_head);
}

// the length build alone, one wave: counts[286] (zeros behind the symbols in use) -> lengths[286]
__global__ void __launch_bounds__(64) k_png_lengths(const uint32_t* __restrict__ counts, int limit, uint32_t* __restrict__ lengths) {
    __shared__ BuildLds s_build;
    const int lane = threadIdx.x;
    uint32_t freq[kPerLane], entry[kPerLane];
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) { const int idx = lane + kLanes * j; freq[j] = idx < png_opt::kSymbols ? counts[idx] : 0u; }
    build_code(freq, png_opt::kSymbols, limit, s_build, entry);
    #pragma unroll
    for (int j = 0; j < kPerLane; ++j) { const int idx = lane + kLanes * j; if (idx < png_opt::kSymbols) lengths[idx] = entry[j] & 15u; }
}

namespace {

// k_png_run_pack's body.  OWN (k_png_opt_pack): a segment whose choice is png_opt::kOwn takes its codes, its header and the header's length from `own`, its table
// in the scratch (own_stride 1), or from the one table of its sequence (k_png_seq_pack: own_stride 0); every other segment, and every segment without OWN, from
// table 0..7's constants.
template <bool OWN>
__device__ __forceinline__ void run_pack(const uint8_t* __restrict__ stream, const uint4* __restrict__ seg_info, const png_opt::OwnTable* __restrict__ own, uint32_t own_stride,
                                         const unsigned long long* __restrict__ seg_start, const uint32_t* __restrict__ meta, uint32_t* __restrict__ frame32, uint32_t n_seg,
                                         unsigned long long n, unsigned long long capacity) {
    __shared__ uint32_t s_image[kRunImageWords];
    __shared__ uint32_t s_code[png_runs::kSymbols];
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_bound[8];
    const int t = threadIdx.x;
    const uint32_t seg = blockIdx.x;
    const uint4 info = seg_info[seg];
    const bool owned = OWN && info.x == (uint32_t)png_opt::kOwn;
    const uint32_t table = info.x & (kTables - 1), bits = info.y;
    if (OWN) own += (size_t)seg * own_stride;
    if (!meta[1] || bits > png_runs::kSegmentBitsMax) return;      // (never: the scan found the frame inside its capacity, and table 7 bounds every block)
    const unsigned long long start = seg_start[seg];
    const size_t first = (size_t)seg * kSegment;
    const uint32_t len = (uint32_t)(n - first < kSegment ? n - first : kSegment);
    const uint32_t off = (uint32_t)start & 31u, n_words = (off + bits + 31) >> 5;
    for (uint32_t i = t; i < n_words; i += kThreads) s_image[i] = 0;
    for (int i = t; i < png_runs::kSymbols; i += kThreads) s_code[i] = owned ? own->code[i] : c_run_codes.e[table][i];
    __syncthreads();
    const uint32_t header_bits = owned ? min(own->header_bits, (uint32_t)png_opt::kOwnHeaderBitsMax) : c_run_block.header[table];
    for (uint32_t i = t; 32 * i < header_bits; i += kThreads) {      // the header, a word per thread (the bits behind H_k are zeros in the table)
        const uint32_t v = (owned ? own->header[i] : c_run_header.e[table][i]) | (i == 0 && seg == n_seg - 1 ? 1u : 0u), p = off + 32 * i;
        atomicOr(&s_image[p >> 5], v << (p & 31));
        if ((p & 31) && (v >> (32 - (p & 31)))) atomicOr(&s_image[(p >> 5) + 1], v >> (32 - (p & 31)));
    }
    const uint32_t at = (uint32_t)t * kBytesPerThread;
    const bool active = at < len;
    RunBytes r{};
    if (active) r = load_run_bytes(stream + first, at, len);
    uint32_t begin = 0, end = 0, count = 0;
    group_run_bounds(active ? last_break(r, at) : 0u, active ? first_break(r, at) : 0xFFFFFFFFu, s_bound, &begin, &end);
    if (active)
        for_each_token(r, at, len, begin, end, [&](uint32_t symbol, uint32_t extra_bits, uint32_t) {
            count += (s_code[symbol] & 15u) + (symbol > (uint32_t)kEob ? extra_bits + 1u : 0u);
        });
    uint32_t all = 0;
    const uint32_t before = group_scan(count, s_part, &all);
    if (active) {
        const uint32_t p = off + header_bits + before;
        uint32_t at_word = p >> 5;
        int n_acc = (int)(p & 31);
        unsigned long long acc = 0;
        auto put = [&](uint32_t value, uint32_t width) {    // at most 15 bits behind fewer than 32 waiting ones
            acc |= (unsigned long long)value << n_acc;
            n_acc += (int)width;
            if (n_acc >= 32) { atomicOr(&s_image[at_word++], (uint32_t)acc); acc >>= 32; n_acc -= 32; }
        };
        for_each_token(r, at, len, begin, end, [&](uint32_t symbol, uint32_t extra_bits, uint32_t extra) {
            const uint32_t e = s_code[symbol];
            put(e >> 4, e & 15u);
            if (symbol > (uint32_t)kEob) put(extra, extra_bits + 1u);      // the extra bits, and the distance code's 0 bit on top of them
        });
        if (at + kBytesPerThread >= len) put(s_code[kEob] >> 4, s_code[kEob] & 15u);      // the thread of the segment's last byte: end-of-block
        if (n_acc) atomicOr(&s_image[at_word], (uint32_t)acc);
    }
    __syncthreads();
    const unsigned long long word0 = start >> 5, word_end = (start + bits) >> 5, cap_words = (capacity + 3) / 4;
    for (uint32_t i = t; i < n_words; i += kThreads) {
        const unsigned long long fw = word0 + i;
        if (fw >= cap_words) continue;
        if (fw == word0 || fw == word_end) atomicOr(&frame32[fw], s_image[i]); else frame32[fw] = s_image[i];
    }
}

}  // namespace

__global__ void __launch_bounds__(kThreads) k_png_run_pack(const uint8_t* __restrict__ stream, const uint4* __restrict__ seg_info, const unsigned long long* __restrict__ seg_start,
                                                           const uint32_t* __restrict__ meta, uint32_t* __restrict__ frame32, uint32_t n_seg, unsigned long long n,
                                                           unsigned long long capacity) {
    run_pack<false>(stream, seg_info, nullptr, 0, seg_start, meta, frame32, n_seg, n, capacity);
}

__global__ void __launch_bounds__(kThreads) k_png_opt_pack(const uint8_t* __restrict__ stream, const uint4* __restrict__ seg_info, const png_opt::OwnTable* __restrict__ own,
                                                           const unsigned long long* __restrict__ seg_start, const uint32_t* __restrict__ meta, uint32_t* __restrict__ frame32,
                                                           uint32_t n_seg, unsigned long long n, unsigned long long capacity) {
    run_pack<true>(stream, seg_info, own, 1, seg_start, meta, frame32, n_seg, n, capacity);
}

// POPPY_FRAME_PNG_SEQ's pack: k_png_opt_pack reading the sequence's one table wherever the choice is 8
__global__ void __launch_bounds__(kThreads) k_png_seq_pack(const uint8_t* __restrict__ stream, const uint4* __restrict__ seg_info, const png_opt::OwnTable* __restrict__ shared,
                                                           const unsigned long long* __restrict__ seg_start, const uint32_t* __restrict__ meta, uint32_t* __restrict__ frame32,
                                                           uint32_t n_seg, unsigned long long n, unsigned long long capacity) {
    run_pack<true>(stream, seg_info, shared, 0, seg_start, meta, frame32, n_seg, n, capacity);
}

__global__ void __launch_bounds__(kThreads) k_png_crc(const uint8_t* __restrict__ frame, const uint32_t* __restrict__ meta, uint32_t* __restrict__ pieces) {
    __shared__ uint32_t s_table[256];
    __shared__ uint32_t s_part[4];
    const int t = threadIdx.x;
    if (!meta[1]) return;
    const long long begin = (long long)kOffIdatType, end = (long long)meta[0] + 4;      // the chunk's type, its data, Adler-32 included
    if ((long long)blockIdx.x * (long long)kCrcBlock >= end - begin) return;
    s_table[t] = c_crc.e[t];
    __syncthreads();
    const long long hi = end - 32ll * ((long long)blockIdx.x * kThreads + t), lo = hi - 32 > begin ? hi - 32 : begin;
    uint32_t c = 0;
    for (long long p = lo; p < hi; ++p) c = s_table[(c ^ frame[p]) & 255u] ^ (c >> 8);
    c = dev_crc_mul(c_crc_shift.e[t], c);
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c ^= __shfl_xor(c, d, 64);
    if ((t & 63) == 0) s_part[t >> 6] = c;
    __syncthreads();
    if (t == 0) pieces[blockIdx.x] = s_part[0] ^ s_part[1] ^ s_part[2] ^ s_part[3];
}

__global__ void __launch_bounds__(kThreads) k_png_finish(const uint32_t* __restrict__ meta, const uint32_t* __restrict__ pieces, uint8_t* __restrict__ frame,
                                                         uint32_t* __restrict__ total_host) {
    __shared__ uint32_t s_part[4];
    const int t = threadIdx.x;
    const bool ok = meta[1] != 0;
    const unsigned long long end = meta[0], length = end + 4 - kOffIdatType;
    const long long n_words = (long long)((length + kCrcBlock - 1) / kCrcBlock);
    uint32_t c = 0;
    if (ok && t < n_words) {                                // words t, t + 256, ..: Horner's rule in x^(8 * kCrcBlock * 256) from the furthest, then word t's own place
        for (long long b = t + (n_words - 1 - t) / kThreads * kThreads; b >= t; b -= kThreads) c = dev_crc_mul(c_crc_block.stride, c) ^ pieces[b];
        c = dev_crc_mul(c_crc_block.e[t], c);
    }
    const uint32_t length_power = wave_x_pow_bytes(length);
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c ^= __shfl_xor(c, d, 64);
    if ((t & 63) == 0) s_part[t >> 6] = c;
    __syncthreads();
    if (t != 0) return;
    uint32_t total = 0;
    if (ok) {
        const uint32_t crc = s_part[0] ^ s_part[1] ^ s_part[2] ^ s_part[3] ^ dev_crc_mul(length_power, 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
        uint8_t* p = frame + end + 4;
        p[0] = (uint8_t)(crc >> 24); p[1] = (uint8_t)(crc >> 16); p[2] = (uint8_t)(crc >> 8); p[3] = (uint8_t)crc;
        total = (uint32_t)(end + kTailBytes);
    }
    if (total_host) { *total_host = total; __threadfence_system(); }
}

size_t png_scratch_bytes(int w, int h, int variant) {
    const size_t n_seg = (size_t)segment_count((size_t)w, (size_t)h);
    return n_seg * (kSegment + sizeof(uint4) + 8) + crc_blocks(w, h, variant) * 4 + 4 * kMetaWords + 16 + (variant == kRunsOwn ? n_seg * sizeof(png_opt::OwnTable) : 0);
}

void launch_png_filter(const uint8_t* bgr, uint8_t* scratch, int w, int h, int variant, hipStream_t s) {
    const bool wide = w % 4 == 0 && (uintptr_t)bgr % 4 == 0;
    hipLaunchKernelGGL(wide ? k_png_filter<true> : k_png_filter<false>, dim3((unsigned)h), dim3(kThreads), 0, s, bgr, scratch_of(scratch, w, h, variant).stream, w);
}
void launch_png_cost(uint8_t* scratch, int w, int h, int variant, hipStream_t s) {
    const Scratch m = scratch_of(scratch, w, h, variant);
    const dim3 grid((unsigned)segment_count((size_t)w, (size_t)h));
    if (variant == kRunsOwn) hipLaunchKernelGGL(k_png_opt_cost, grid, dim3(kThreads), 0, s, (const uint8_t*)m.stream, m.seg, m.own, stream_bytes((size_t)w, (size_t)h));
    else hipLaunchKernelGGL(variant == kRuns ? k_png_run_cost : k_png_cost, grid, dim3(kThreads), 0, s, (const uint8_t*)m.stream, m.seg, stream_bytes((size_t)w, (size_t)h));
}
void launch_png_scan(uint8_t* scratch, uint8_t* frame, int w, int h, int variant, hipStream_t s) {
    const Scratch m = scratch_of(scratch, w, h, variant);
    constexpr CrcTable table = make_crc_table();
    const uint8_t ihdr[17] = {'I', 'H', 'D', 'R', (uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w,
                              (uint8_t)(h >> 24), (uint8_t)(h >> 16), (uint8_t)(h >> 8), (uint8_t)h, 8, 2, 0, 0, 0};
    uint32_t c = 0xFFFFFFFFu;
    for (uint8_t byte : ihdr) c = table.e[(c ^ byte) & 255u] ^ (c >> 8);
    hipLaunchKernelGGL(k_png_scan, dim3(1), dim3(kThreads), 0, s, (const uint4*)m.seg, m.start, m.meta, (uint32_t*)frame, (uint32_t)segment_count((size_t)w, (size_t)h),
                       stream_bytes((size_t)w, (size_t)h), (uint32_t)w, (uint32_t)h, c ^ 0xFFFFFFFFu, capacity_of(w, h, variant));
}
void launch_png_pack(const uint8_t* scratch, uint8_t* frame, int w, int h, int variant, hipStream_t s) {
    const Scratch m = scratch_of(const_cast<uint8_t*>(scratch), w, h, variant);
    const uint32_t n_seg = (uint32_t)segment_count((size_t)w, (size_t)h);
    if (variant == kRunsOwn)
        hipLaunchKernelGGL(k_png_opt_pack, dim3(n_seg), dim3(kThreads), 0, s, (const uint8_t*)m.stream, (const uint4*)m.seg, (const png_opt::OwnTable*)m.own, (const unsigned long long*)m.start,
                           (const uint32_t*)m.meta, (uint32_t*)frame, n_seg, stream_bytes((size_t)w, (size_t)h), capacity_of(w, h, variant));
    else
        hipLaunchKernelGGL(variant == kRuns ? k_png_run_pack : k_png_pack, dim3(n_seg), dim3(kThreads), 0, s, (const uint8_t*)m.stream, (const uint4*)m.seg, (const unsigned long long*)m.start,
                           (const uint32_t*)m.meta, (uint32_t*)frame, n_seg, stream_bytes((size_t)w, (size_t)h), capacity_of(w, h, variant));
}
void launch_png_crc(uint8_t* scratch, const uint8_t* frame, int w, int h, int variant, hipStream_t s) {
    const Scratch m = scratch_of(scratch, w, h, variant);
    hipLaunchKernelGGL(k_png_crc, dim3((unsigned)crc_blocks(w, h, variant)), dim3(kThreads), 0, s, frame, (const uint32_t*)m.meta, m.crc);
}
void launch_png_finish(const uint8_t* scratch, uint8_t* frame, uint32_t* total_host, int w, int h, int variant, hipStream_t s, hipEvent_t done) {
    const Scratch m = scratch_of(const_cast<uint8_t*>(scratch), w, h, variant);
    hipExtLaunchKernelGGL(k_png_finish, dim3(1), dim3(kThreads), 0, s, nullptr, done, 0, (const uint32_t*)m.meta, (const uint32_t*)m.crc, frame, total_host);
}

void launch_png_seq_count(const uint8_t* place, uint32_t* sums, int w, int h, hipStream_t s, hipEvent_t done) {
    const Scratch m = scratch_of(const_cast<uint8_t*>(place), w, h, kRunsSeq);
    hipExtLaunchKernelGGL(k_png_seq_count, dim3((unsigned)segment_count((size_t)w, (size_t)h)), dim3(kThreads), 0, s, nullptr, done, 0, (const uint8_t*)m.stream, sums, stream_bytes((size_t)w, (size_t)h));
}
void launch_png_seq_table(uint32_t* sums, void* table, hipStream_t s) {
    hipLaunchKernelGGL(k_png_seq_table, dim3(1), dim3(kLanes), 0, s, sums, (png_opt::OwnTable*)table);
}
void launch_png_seq_cost(uint8_t* place, const void* table, int w, int h, hipStream_t s) {
    const Scratch m = scratch_of(place, w, h, kRunsSeq);
    hipLaunchKernelGGL(k_png_seq_cost, dim3((unsigned)segment_count((size_t)w, (size_t)h)), dim3(kThreads), 0, s, (const uint8_t*)m.stream, m.seg, (const png_opt::OwnTable*)table, stream_bytes((size_t)w, (size_t)h));
}
void launch_png_seq_pack(const uint8_t* place, const void* table, uint8_t* frame, int w, int h, hipStream_t s) {
    const Scratch m = scratch_of(const_cast<uint8_t*>(place), w, h, kRunsSeq);
    const uint32_t n_seg = (uint32_t)segment_count((size_t)w, (size_t)h);
    hipLaunchKernelGGL(k_png_seq_pack, dim3(n_seg), dim3(kThreads), 0, s, (const uint8_t*)m.stream, (const uint4*)m.seg, (const png_opt::OwnTable*)table, (const unsigned long long*)m.start,
                       (const uint32_t*)m.meta, (uint32_t*)frame, n_seg, stream_bytes((size_t)w, (size_t)h), capacity_of(w, h, kRunsSeq));
}

void launch_png_length_build(const uint32_t* counts, int limit, uint32_t* lengths, hipStream_t s) {
    hipLaunchKernelGGL(k_png_lengths, dim3(1), dim3(64), 0, s, counts, limit, lengths);
}

}  // namespace poppy_hip
