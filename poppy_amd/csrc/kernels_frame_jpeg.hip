// kernels_frame_jpeg.hip — an I420 frame on the device (kernels_frame_format.hip) -> POPPY_FRAME_JPEG for the writer hand-off (include/poppy_hip.h has the rule):
// one baseline JFIF file, coded in independent restart intervals of POPPY_JPEG_RESTART_MCUS MCUs.  poppy_i420_to_jpeg_frame (frame_jpeg.cpp) is the host
// statement; the bytes are equal.  The same two kernels code POPPY_FRAME_JPEG444 from the I444 planes (kernels_frame_i444.hip; poppy_i444_to_jpeg_frame): the
// coder is a template over the sampling (jpeg_tables.h: Sampling), which decides the blocks of an MCU (6 or 3), the MCUs of a segment (8 or 16: 48 lanes
// either way), each block's plane and origin and which lane holds the previous block of the same component.  Everything behind the DC difference is one code.
//
// Two dispatches behind k_bgr_to_i420, no host round trip:
//   k_jpeg_code  a segment per wave, a workgroup of one wave (no workgroup barrier).  Nothing in a segment is serial but the bit positions, so a LANE takes a BLOCK:
//                the segment's 8 MCUs are 48 blocks, lane = 6 * MCU + block.  A lane reads its 64 samples (coordinates clamped), runs the two DCT passes in
//                registers — fully unrolled, the table's even / odd symmetry halving the multiplications, the same integers as the table form since nothing
//                overflows —, quantises with a multiply-high by the divisor's reciprocal (jpeg_tables.h proves it equal to the division) and stores the 64
//                coefficients in zig-zag order into LDS, transposed ([position][lane], so that the lanes of a wave read one row).  The DC difference comes from
//                the previous block of the same component by a shuffle.  The Huffman coding then runs twice over the lane's coefficients with a uniform trip
//                count of 63: once to count the block's bits, and, after a wave prefix sum over the counts has placed every block, once to OR the codes into the
//                segment's bit buffer in LDS at their final positions (ds_or_b32; a code of at most 26 bits touches at most two words, and neighbouring blocks
//                share at most their boundary words).  Lane 0 adds the padding 1-bits.  Stuffing is a second count-and-scan, over bytes: 64 bytes per step, a
//                ballot of the FF bytes and a population count below the lane give every byte its place; the bytes go to the segment's fixed slot of the
//                scratch buffer (kJpegSlotBytes apart) and lane 0 stores the byte length.
//   k_jpeg_pack  every workgroup sums the lengths in front of its group of segments (each with its 2 marker bytes) and all of them for `total`, as k_gif_pack
//                does, then moves its segments' bytes to their place and writes RST(k mod 8) behind each, EOI behind the last.  Workgroup 0 writes the header —
//                the context's bytes for the quality, with width and height filled in — and `total`, into the frame and into a word of mapped pinned host memory.
//
// POPPY_FRAME_JPEG_OPT and POPPY_FRAME_JPEG444_OPT (the same files on Huffman tables built from the frame's own symbol counts) are four dispatches, no host round trip:
//   k_jpeg_count   k_jpeg_code's front end (block_front: samples, DCT, quantiser, DC difference) and its walk over the block's symbols (walk_block), adding every
//                  symbol into the workgroup's count tables in LDS (ds_add).  A workgroup is four waves, a wave takes a segment at a time and every fourth group of
//                  the grid's; at the end the workgroup adds its non-zero counts into the frame's table with one integer atomic each (at most kCountGroupsMax
//                  workgroups on 544 words, of which a frame uses 100 to 300).  Integer adds: the counts are exact whatever the schedule.  The frame's table is
//                  zero in front of the pass: the scratch's owner clears it once (launch_jpeg_counts_clear), k_jpeg_tables clears what it has read.
//   k_jpeg_tables  one workgroup, a wave per table (DC 0, AC 0, DC 1, AC 1).  The wave reads its table's counts and stores zeros — a lane holds symbols lane + 64 j, lane 0 the
//                  reserved entry 256 as well — and runs the rule's merges in registers: the two smallest non-zero counts are the minima of a packed key
//                  (count << 9 | 511 - symbol: the larger symbol wins a tie), taken with ds_min_u64 on two LDS words, and a merge is every lane's update of
//                  "symbols whose tree is c1 or c2".  Lengths are counted in LDS, lane 0 runs Annex K.3 from the longest length that occurs, a symbol's place in
//                  the DHT is the number of smaller (length, symbol) keys, and its canonical code follows from its place.  Out come the lookup entries the coder
//                  reads and each table's DHT bytes (jpeg_tables.h: OptTables).
//   k_jpeg_code    as above, its Huffman entries read from the frame's built tables in device memory (template parameter OPT), its bit buffer and scratch slot at
//                  the OPT bound (a DC code may have 12 bits).
//   k_jpeg_pack    as above; its OPT form puts the header together from the fixed header's bytes around the built DHT, and the data behind it, wherever it ends.
//
// POPPY_FRAME_JPEG and POPPY_FRAME_JPEG444 under a byte budget (poppy_hip_set_jpeg_budget; frame_jpeg_budget.cpp is the host statement) put kJpegBudgetSteps pairs of
// dispatches in front of the two, no host round trip:
//   k_jpeg_measure k_jpeg_code without its stores, at the qualities of one step of the search: the samples and the DCT once (block_dct), the 64 coefficients in front of
//                  the quantiser kept in the lane's registers, and per quality the quantiser (block_quantise), the bit string in LDS (segment_bits) and the count of its
//                  FF bytes: every segment's exact byte length at that quality.  The tables of all 100 qualities, the budget and the highest quality are device memory.
//   k_jpeg_pick    one workgroup: the file's size at each measured quality, the search's interval advanced by the rule; at its end the picked quality, in the scratch.
//   k_jpeg_code, k_jpeg_pack   once, on the picked quality's entry of the 100 tables (an index read from the scratch).
//
// The same two formats under a SEQUENCE budget (poppy_hip_set_jpeg_sequence_budget; frame_jpeg_seq_budget.cpp is the host statement) run ONE search for all the
// frames of a sequence, which wait as planes in a store: per step one k_jpeg_measure over segments x frames (blockIdx.y: the frame) and one k_jpeg_pick that sums
// every frame's lengths per quality in 64 bits against the 64-bit budget of JpegSeqBudgetParams; the search's state is the sequence's, not a frame's scratch, and
// every frame's k_jpeg_code and k_jpeg_pack then read the picked quality from there.
#include "kernels.h"
#include <hip/hip_ext.h>
#include <algorithm>
#include <utility>

namespace poppy_hip {

namespace {

using namespace jpeg;

constexpr int kSegLanes = 6 * kRestartMcus;                 // blocks of a full segment
static_assert(kSegLanes <= 64, "a segment's blocks are the lanes of one wave");
static_assert(mcu_blocks(k444) * kRestartMcus444 == kSegLanes, "... of either sampling: the bit buffer and the scratch slot below are sized for them");
constexpr int kBitWords = (int)((6 * kBlockBitsMax * kRestartMcus + 31) / 32) + 2;      // the segment's bits at their bound, the word a code may spill into
static_assert(kJpegSlotBytes >= 2 * ((6 * kBlockBitsMax * kRestartMcus + 7) / 8), "a slot holds a segment with every byte stuffed");
constexpr int kOptBitWords = (int)((6 * kOptBlockBitsMax * kRestartMcus + 31) / 32) + 2;      // ... on per-frame tables, where a DC code may have 12 bits
static_assert(kJpegOptSlotBytes >= 2 * ((6 * kOptBlockBitsMax * kRestartMcus + 7) / 8), "an OPT slot holds a segment with every byte stuffed");

__constant__ HuffTables c_huff = make_huff();

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// one output of the 8-point transform from the four sums (even U) or differences (odd U) of the mirrored inputs: T[U][7 - x] = (-1)^U T[U][x]
template <int U, int SHIFT>
__device__ __forceinline__ int dct_out(const int (&e)[4]) {
    constexpr int c0 = dct_entry(U, 0), c1 = dct_entry(U, 1), c2 = dct_entry(U, 2), c3 = dct_entry(U, 3);
    return (c0 * e[0] + c1 * e[1] + c2 * e[2] + c3 * e[3] + (1 << (SHIFT - 1))) >> SHIFT;
}
template <int SHIFT>
__device__ __forceinline__ void dct8(int (&v)[8]) {
    const int s[4] = {v[0] + v[7], v[1] + v[6], v[2] + v[5], v[3] + v[4]};
    const int d[4] = {v[0] - v[7], v[1] - v[6], v[2] - v[5], v[3] - v[4]};
    v[0] = dct_out<0, SHIFT>(s); v[1] = dct_out<1, SHIFT>(d); v[2] = dct_out<2, SHIFT>(s); v[3] = dct_out<3, SHIFT>(d);
    v[4] = dct_out<4, SHIFT>(s); v[5] = dct_out<5, SHIFT>(d); v[6] = dct_out<6, SHIFT>(s); v[7] = dct_out<7, SHIFT>(d);
}

constexpr int zigzag_position(int natural) {
    for (int k = 0; k < 64; ++k) if (kZigzag[k] == natural) return k;
    return -1;
}

// what the front end of a segment works in (one per wave)
struct FrontLds {
    int16_t coef[64][64];                                   // [zig-zag position][lane]
    uint2 q[2][64];                                         // per table and natural index: the bias 4 Q, the reciprocal of 8 Q
};
template <int WORDS>
struct CoderLds {
    FrontLds f;
    uint32_t bits[WORDS];                                   // the segment's bit string, most significant bit of word 0 first
    uint32_t ac[2][256];
    uint32_t dc[2][16];
};

// coefficient N of the lane's block: quantised, into its zig-zag row; returns it
template <int N>
__device__ __forceinline__ int quantise_store(FrontLds& L, int F, int table, int lane) {
    constexpr int pos = zigzag_position(N);
    const uint2 q = L.q[table][N];
    const uint32_t a = (uint32_t)(F < 0 ? -F : F);
    const int m = (int)__umulhi(a + q.x, q.y);
    const int v = F < 0 ? -m : m;
    L.coef[pos][lane] = (int16_t)v;
    return v;
}
template <int... N>
__device__ __forceinline__ int quantise_block(FrontLds& L, const int (&f)[64], int table, int lane, std::integer_sequence<int, N...>) {
    int dc = 0;
    ((N == 0 ? (void)(dc = quantise_store<N>(L, f[N], table, lane)) : (void)quantise_store<N>(L, f[N], table, lane)), ...);
    return dc;
}

// `len` bits (1..26: an AC code of at most 16 bits with 10 value bits; a DC code with its value is 11 + 11, on per-frame tables 12 + 11), right-aligned in
// `value`, at bit position `at` of the segment
__device__ __forceinline__ void emit_bits(uint32_t* bits, uint32_t at, uint32_t value, int len) {
    const uint32_t word = at >> 5, off = at & 31;
    const unsigned long long x = (unsigned long long)value << (64 - (int)off - len);
    atomicOr(&bits[word], (uint32_t)(x >> 32));
    if (off + (uint32_t)len > 32) atomicOr(&bits[word + 1], (uint32_t)x);
}

__device__ __forceinline__ int category(int v) { return 32 - __clz(v < 0 ? -v : v); }      // (__clz(0) is 32)

// The lane's block as its symbols, the one walk of the counting and the coding passes: put(is_dc, symbol, value, category) for the DC category, then per AC
// symbol (ZRL and EOB: value 0, category 0).
template <class Put>
__device__ __forceinline__ void walk_block(const FrontLds& L, int lane, int diff, Put put) {
    { const int cat = category(diff); put(true, cat, diff, cat); }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = L.coef[k][lane];
        if (v == 0) { ++run; continue; }
        for (; run >= 16; run -= 16) put(false, 0xF0, 0, 0);
        const int cat = category(v);
        put(false, run << 4 | cat, v, cat);
        run = 0;
    }
    if (run) put(false, 0, 0, 0);
}

// The lane's block as Huffman codes: counted (EMIT false) or ORed into the bit buffer from position `at` on.  Returns the block's bits.
template <bool EMIT, int WORDS>
__device__ __forceinline__ uint32_t code_block(CoderLds<WORDS>& L, int lane, int table, int diff, uint32_t at) {
    uint32_t n = 0;
    walk_block(L.f, lane, diff, [&](bool is_dc, int symbol, int v, int cat) {      // a symbol's code, then the value's low `cat` bits
        const uint32_t huff = is_dc ? L.dc[table][symbol] : L.ac[table][symbol];
        const int len = (int)(huff & 255) + cat;
        if (EMIT) emit_bits(L.bits, at + n, (huff >> 8) << cat | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1)), len);
        n += (uint32_t)len;
    });
    return n;
}

// A segment's front end, the lane's block of it: samples -> DCT -> quantiser (the coefficients into L.coef) -> DC difference by shuffle.  Every lane of the wave
// calls it; L.q holds the quantiser.
struct BlockFront {
    bool active;                                            // the lane has a block (the frame's last segment may be short)
    int table;                                              // 0: luma, 1: chroma
    int diff;                                               // the DC difference
};
// ... in its parts (k_jpeg_measure runs the first once and the other two per quality).  block_dct: which block the lane has, and its 64 coefficients in front of
// the quantiser, natural order, in f (registers)
struct BlockPlace {
    bool active;
    int table;
    int b, m_in;                                            // the block's number in its MCU, the MCU's in the segment
};
template <Sampling S>
__device__ __forceinline__ BlockPlace block_dct(int (&f)[64], const uint8_t* __restrict__ i420, int seg, int lane, int w, int h, int mw, int n_mcu) {
    constexpr int kBlocks = mcu_blocks(S), kMcus = restart_mcus(S);
    const int first = seg * kMcus, mcus = min(kMcus, n_mcu - first);
    const int m_in = lane / kBlocks, b = lane - kBlocks * m_in, table = S == k444 ? b >= 1 : b >= 4;
    const bool active = m_in < mcus;
    if (active) {
        const int m = first + m_in, my = m / mw, mx = m - my * mw;
        // the block's plane, that plane's size and the block's origin in it.  4:4:4: (the I444 planes) every plane w x h, every block at (8 mx, 8 my)
        const int cw = S == k444 ? w : (w + 1) / 2, ch = S == k444 ? h : (h + 1) / 2;
        const int pw = table ? cw : w, ph = table ? ch : h;
        const int x0 = table || S == k444 ? 8 * mx : 16 * mx + 8 * (b & 1), y0 = table || S == k444 ? 8 * my : 16 * my + 8 * (b >> 1);
        const uint8_t* plane = i420 + (!table ? (size_t)0 : (size_t)w * h + (b == kBlocks - 1 ? (size_t)cw * ch : (size_t)0));
        #pragma unroll
        for (int y = 0; y < 8; ++y) {
            const uint8_t* row = plane + (size_t)min(y0 + y, ph - 1) * pw;
            #pragma unroll
            for (int x = 0; x < 8; ++x) f[y * 8 + x] = (int)row[min(x0 + x, pw - 1)] - 128;
        }
        #pragma unroll
        for (int y = 0; y < 8; ++y) {                       // rows: t(y, u)
            int v[8];
            #pragma unroll
            for (int x = 0; x < 8; ++x) v[x] = f[y * 8 + x];
            dct8<kDctPass1Shift>(v);
            #pragma unroll
            for (int x = 0; x < 8; ++x) f[y * 8 + x] = v[x];
        }
        #pragma unroll
        for (int u = 0; u < 8; ++u) {                       // columns: F(v, u)
            int v[8];
            #pragma unroll
            for (int y = 0; y < 8; ++y) v[y] = f[y * 8 + u];
            dct8<kDctPass2Shift>(v);
            #pragma unroll
            for (int y = 0; y < 8; ++y) f[y * 8 + u] = v[y];
        }
    }
    return BlockPlace{active, table, b, m_in};
}
// the quantiser in L.q on f (the coefficients into L.coef) and the DC difference by shuffle; every lane of the wave calls it
template <Sampling S>
__device__ __forceinline__ int block_quantise(FrontLds& L, const int (&f)[64], const BlockPlace& p, int lane) {
    const int b = p.b;
    const int dc = p.active ? quantise_block(L, f, p.table, lane, std::make_integer_sequence<int, 64>()) : 0;
    // the previous block of the same component: the luma block before, Y11 of the MCU before for Y00, the same chroma block of the MCU before; the segment's first: 0
    // (4:4:4: the same block of the MCU before, three lanes down)
    const int from = S == k444 ? lane - 3 : b >= 4 ? lane - 6 : b == 0 ? lane - 3 : lane - 1;
    const int before = __shfl(dc, max(from, 0), 64);
    return dc - ((S == k444 || b == 0 || b >= 4) && p.m_in == 0 ? 0 : before);
}
template <Sampling S>
__device__ __forceinline__ BlockFront block_front(FrontLds& L, const uint8_t* __restrict__ i420, int seg, int lane, int w, int h, int mw, int n_mcu) {
    int f[64];
    const BlockPlace p = block_dct<S>(f, i420, seg, lane, w, h, mw, n_mcu);
    return BlockFront{p.active, p.table, block_quantise<S>(L, f, p, lane)};
}

// A segment's bit string from its front end: every block counted, placed by a wave prefix sum and ORed into L.bits, the padding 1-bits behind; returns the
// string's length in bits.  Every lane of the wave calls it.
template <int WORDS>
__device__ __forceinline__ uint32_t segment_bits(CoderLds<WORDS>& L, int lane, bool active, int table, int diff) {
    const uint32_t n_bits = active ? code_block<false>(L, lane, table, diff, 0) : 0;
    uint32_t incl = n_bits;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
    const uint32_t total_bits = __shfl(incl, 63, 64);
    for (uint32_t i = lane; i < (total_bits + 31) / 32 + 1; i += 64) L.bits[i] = 0;
    wave_sync();
    if (active) code_block<true>(L, lane, table, diff, incl - n_bits);
    const int pad = (int)((8 - (total_bits & 7)) & 7);
    if (lane == 0 && pad) emit_bits(L.bits, total_bits, (1u << pad) - 1, pad);
    wave_sync();
    return total_bits;
}

// ---- the byte budget (include/poppy_hip.h, "JPEG byte budget"): the search's state, in the frame's scratch.  Nothing of it is a kernel argument that a captured
// body could keep: the budget and the highest quality are read from JpegBudgetParams in device memory, the state from here. ----
struct BudgetSearch {
    uint32_t lo, hi;                                        // hi is known not to fit; lo = 0: nothing known to fit
    uint32_t picked;                                        // 0 while the search runs, then the frame's quality
    uint32_t pad;
};
// the quality that k_jpeg_code and k_jpeg_pack index the tables by (whatever the word holds, the index stays inside the 100 tables)
__device__ __forceinline__ int picked_quality(const BudgetSearch* s) { return (int)min(max(s->picked, 1u), 100u); }

// The qualities a step measures: the first kJpegBudgetLevels levels of the search tree below (lo, hi) in breadth-first order, and at step 0, where
// (lo, hi) = (0, quality_max), quality_max in front.  fits(q) is a pure function of the frame, so measuring a level whose question the level above has not
// answered yet changes no result.  k_jpeg_measure and k_jpeg_pick derive the same list from the same state.
constexpr int kBudgetListMax = kJpegBudgetListMax;
static_assert(kJpegBudgetLevels == 1 || kJpegBudgetLevels == 2, "probe_list writes out one or two levels");
static_assert(kBudgetListMax == (1 << kJpegBudgetLevels), "a full tree of the step's levels, and quality_max at step 0");
__device__ __forceinline__ int probe_list(int lo, int hi, bool first, int (&q)[kBudgetListMax]) {
    int n = 0;
    if (first) q[n++] = hi;
    if (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        q[n++] = mid;
        if (kJpegBudgetLevels > 1) {
            if (mid - lo > 1) q[n++] = (lo + mid) >> 1;
            if (hi - mid > 1) q[n++] = (mid + hi) >> 1;
        }
    }
    return n;
}
// the state a step starts from: step 0 from the context's highest quality (clamped: whatever the words hold, every table index stays inside the 100), later steps
// from what the pick before left.  False: the search is over.
__device__ __forceinline__ bool search_state(const JpegBudgetParams* params, const BudgetSearch* search, bool first, int* lo, int* hi) {
    if (first) { *lo = 0; *hi = (int)min(max(params->quality_max, 1u), 100u); return true; }
    if (search->picked) return false;
    *lo = (int)min(search->lo, 99u); *hi = (int)min(max(search->hi, (uint32_t)*lo + 1), 100u);
    return true;
}

}  // namespace

// OPT: the Huffman entries are the frame's built tables (`huff`, device memory: k_jpeg_tables wrote them) instead of the Annex K ones, and the bit buffer and the
// scratch slots are the OPT bound's
template <Sampling S, bool OPT>
__global__ void __launch_bounds__(64) k_jpeg_code(const uint8_t* __restrict__ i420, const QualityTables* __restrict__ tables, const HuffTables* __restrict__ huff,
                                                  uint8_t* __restrict__ scratch, uint32_t* __restrict__ lengths, int w, int h, int mw, int n_mcu, const BudgetSearch* __restrict__ search) {
    __shared__ CoderLds<OPT ? kOptBitWords : kBitWords> L;
    const int lane = threadIdx.x, seg = blockIdx.x;
    if (search) tables += picked_quality(search) - 1;      // under a byte budget `tables` are all 100 qualities' and k_jpeg_pick chose one
    if constexpr (OPT) {
        for (int i = lane; i < 512; i += 64) L.ac[i >> 8][i & 255] = huff->ac[i >> 8][i & 255];
        if (lane < 32) L.dc[lane >> 4][lane & 15] = huff->dc[lane >> 4][lane & 15];
    } else {
        for (int i = lane; i < 512; i += 64) L.ac[i >> 8][i & 255] = c_huff.ac[i >> 8][i & 255];
        if (lane < 32) L.dc[lane >> 4][lane & 15] = c_huff.dc[lane >> 4][lane & 15];
    }
    for (int i = lane; i < 128; i += 64) L.f.q[i >> 6][i & 63] = make_uint2(tables->bias[i >> 6][i & 63], tables->recip[i >> 6][i & 63]);
    wave_sync();
    const BlockFront front = block_front<S>(L.f, i420, seg, lane, w, h, mw, n_mcu);
    const uint32_t total_bits = segment_bits(L, lane, front.active, front.table, front.diff);
    // byte stuffing: byte i of the string goes to i + (the FF bytes in front of it), a zero byte behind every FF
    const uint32_t n_bytes = (total_bits + 7) / 8;
    uint8_t* dst = scratch + (size_t)seg * (OPT ? kJpegOptSlotBytes : kJpegSlotBytes);
    uint32_t n_ff = 0;
    for (uint32_t base = 0; base < n_bytes; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < n_bytes;
        const uint32_t byte = valid ? (L.bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u : 0u;
        const unsigned long long ff = __ballot(valid && byte == 255u);
        const uint32_t at = i + n_ff + (uint32_t)__popcll(ff & ((1ull << lane) - 1));
        if (valid) { dst[at] = (uint8_t)byte; if (byte == 255u) dst[at + 1] = 0; }
        n_ff += (uint32_t)__popcll(ff);
    }
    if (lane == 0) lengths[seg] = n_bytes + n_ff;
}

// The coder without its stores, at the qualities of one step of the budget's search (probe_list): a segment per wave and a block per lane as in k_jpeg_code, the
// samples and the DCT once, the 64 coefficients in front of the quantiser kept in the lane's registers, and per quality the quantiser, the bit string in LDS and
// the count of its FF bytes — the segment's exact byte length, into measured[(k * n_frames + frame) * n_seg + seg].  `tables`: all 100 qualities'.
// A frame alone: n_frames 1 on a grid of n_seg.  A sequence's store: the grid is n_seg x frames, frame frame0 + blockIdx.y has its planes frame_stride bytes
// behind the frame before it.
template <Sampling S>
__global__ void __launch_bounds__(64) k_jpeg_measure(const uint8_t* __restrict__ i420, const QualityTables* __restrict__ tables, const JpegBudgetParams* __restrict__ params,
                                                     const BudgetSearch* __restrict__ search, uint32_t* __restrict__ measured, int first, int w, int h, int mw, int n_mcu, int n_seg,
                                                     size_t frame_stride, int frame0, int n_frames) {
    __shared__ CoderLds<kBitWords> L;
    const int lane = threadIdx.x, seg = blockIdx.x, frame = frame0 + (int)blockIdx.y;
    i420 += (size_t)frame * frame_stride;
    int lo, hi, list[kBudgetListMax];
    if (!search_state(params, search, first != 0, &lo, &hi)) return;      // (uniform: the search is over)
    const int n = probe_list(lo, hi, first != 0, list);
    if (n == 0) return;
    for (int i = lane; i < 512; i += 64) L.ac[i >> 8][i & 255] = c_huff.ac[i >> 8][i & 255];
    if (lane < 32) L.dc[lane >> 4][lane & 15] = c_huff.dc[lane >> 4][lane & 15];
    int f[64];
    const BlockPlace place = block_dct<S>(f, i420, seg, lane, w, h, mw, n_mcu);
    for (int k = 0; k < n; ++k) {
        const QualityTables* t = tables + (list[k] - 1);
        for (int i = lane; i < 128; i += 64) L.f.q[i >> 6][i & 63] = make_uint2(t->bias[i >> 6][i & 63], t->recip[i >> 6][i & 63]);
        wave_sync();
        const int diff = block_quantise<S>(L.f, f, place, lane);
        const uint32_t total_bits = segment_bits(L, lane, place.active, place.table, diff);
        const uint32_t n_bytes = (total_bits + 7) / 8;
        uint32_t n_ff = 0;
        for (uint32_t base = 0; base < n_bytes; base += 64) {
            const uint32_t i = base + lane;
            const uint32_t byte = i < n_bytes ? (L.bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u : 0u;
            n_ff += (uint32_t)__popcll(__ballot(byte == 255u));
        }
        if (lane == 0) measured[((size_t)k * n_frames + frame) * n_seg + seg] = n_bytes + n_ff;
        wave_sync();                                        // (the next quality's quantiser, coefficients and bits go where this one's were read)
    }
}

// One workgroup: size(q) of every quality the step measured — the header, the segments' lengths with their two marker bytes each; the file, not `total` — and
// the search advanced by the rule over the step's levels.  Leaves the next step's (lo, hi), or the frame's quality in `picked`.
// SEQ: size(q) is the sum over the n_frames frames of a sequence (n_frames headers, n_frames x n_seg lengths per quality, integers: no order changes the sum) and the
// budget is the 64 bits of JpegSeqBudgetParams, whose first two words are laid out as JpegBudgetParams' (search_state reads the highest quality from either).
template <bool SEQ>
__global__ void __launch_bounds__(256) k_jpeg_pick(const JpegBudgetParams* __restrict__ params, BudgetSearch* __restrict__ search, const uint32_t* __restrict__ measured,
                                                   int first, int n_seg, int n_frames) {
    __shared__ unsigned long long s_part[kBudgetListMax][4];
    int lo, hi, list[kBudgetListMax];
    if (!search_state(params, search, first != 0, &lo, &hi)) return;
    const int n = probe_list(lo, hi, first != 0, list);
    const int t = threadIdx.x;
    for (int k = 0; k < n; ++k) {
        unsigned long long sum = 0;
        const size_t n_len = (size_t)(SEQ ? n_frames : 1) * (size_t)n_seg;
        for (size_t i = t; i < n_len; i += 256) sum += measured[(size_t)k * n_len + i] + 2;
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if ((t & 63) == 0) s_part[k][t >> 6] = sum;
    }
    __syncthreads();
    if (t != 0) return;
    unsigned long long budget = params->budget, headers = kHeaderBytes;
    if constexpr (SEQ) {
        const JpegSeqBudgetParams* sp = (const JpegSeqBudgetParams*)params;
        budget = (unsigned long long)sp->budget_low | (unsigned long long)sp->budget_high << 32;
        headers = (unsigned long long)kHeaderBytes * (unsigned long long)n_frames;
    }
    auto fits = [&](int q) {                                // (q is in the list: the list is the tree's levels that the walk below takes)
        for (int k = 0; k < n; ++k) if (list[k] == q) return headers + s_part[k][0] + s_part[k][1] + s_part[k][2] + s_part[k][3] <= budget;
        return false;
    };
    uint32_t picked = 0;
    if (first && fits(hi)) picked = (uint32_t)hi;
    else {
        for (int level = 0; level < kJpegBudgetLevels && hi - lo > 1; ++level) {
            const int mid = (lo + hi) >> 1;
            if (fits(mid)) lo = mid; else hi = mid;
        }
        if (hi - lo <= 1) picked = (uint32_t)max(lo, 1);
    }
    search->lo = (uint32_t)lo; search->hi = (uint32_t)hi; search->picked = picked;
}

namespace {
constexpr int kCountWaves = 4;                              // segments a counting workgroup has in flight
constexpr int kCountGroupsMax = 256;                        // ... and the most workgroups, so the most that add into one word of the frame's counts
struct CountLds {
    FrontLds f[kCountWaves];
    uint32_t n[kCountWords];                                // the workgroup's counts (jpeg_tables.h: SymbolCounts)
};
}

template <Sampling S>
__global__ void __launch_bounds__(64 * kCountWaves) k_jpeg_count(const uint8_t* __restrict__ i420, const QualityTables* __restrict__ tables, uint32_t* __restrict__ counts,
                                                                int w, int h, int mw, int n_mcu, int n_seg) {
    __shared__ CountLds L;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    for (int i = t; i < kCountWords; i += 64 * kCountWaves) L.n[i] = 0;
    FrontLds& F = L.f[wave];
    for (int i = lane; i < 128; i += 64) F.q[i >> 6][i & 63] = make_uint2(tables->bias[i >> 6][i & 63], tables->recip[i >> 6][i & 63]);
    __syncthreads();
    for (int seg = blockIdx.x * kCountWaves + wave; seg < n_seg; seg += gridDim.x * kCountWaves) {      // (wave-uniform: every lane of the wave makes every trip)
        const BlockFront front = block_front<S>(F, i420, seg, lane, w, h, mw, n_mcu);
        uint32_t* dc = L.n + 16 * front.table;
        uint32_t* ac = L.n + 32 + 256 * front.table;
        if (front.active) walk_block(F, lane, front.diff, [&](bool is_dc, int symbol, int, int) { atomicAdd(is_dc ? &dc[symbol] : &ac[symbol], 1u); });
        wave_sync();                                        // (the next trip's coefficients go where this trip's were read)
    }
    __syncthreads();
    for (int i = t; i < kCountWords; i += 64 * kCountWaves) if (const uint32_t n = L.n[i]) atomicAdd(&counts[i], n);
}

namespace {
struct BuildLds {
    uint32_t of_length[4][260];                             // per table: the symbols of each length 0..257
    uint32_t key[4][256];                                   // ... a symbol's (length before limiting) << 8 | symbol, ~0 without a code
    unsigned long long pick[4][2];                          // ... the two smallest keys of the merge at hand
    uint32_t first_code[4][17], first_place[4][17], codes[4][17];      // ... per limited length: its first canonical code, the place of its first symbol, its symbols
};
constexpr unsigned long long kNoKey = ~0ull;
}

// The table rule (include/poppy_hip.h) on a frame's counts, a wave per DHT table; `out`: the lookup entries and the DHT bytes.  The counts are zero afterwards.
__global__ void __launch_bounds__(256) k_jpeg_tables(uint32_t* __restrict__ counts, OptTables* __restrict__ out) {
    __shared__ BuildLds L;
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n_sym = table_symbols(k);
    uint32_t* src = counts + (k & 1 ? 32 + 256 * (k >> 1) : 16 * (k >> 1));
    uint32_t freq[5];
    int tree[5], len[5];
    #pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int idx = lane + 64 * j;
        uint32_t f = 0;
        if (idx < n_sym) { f = src[idx]; src[idx] = 0; }
        freq[j] = idx == 256 ? 1u : f;                      // the reserved entry
        tree[j] = idx; len[j] = 0;
    }
    for (int i = lane; i < 260; i += 64) L.of_length[k][i] = 0;
    volatile unsigned long long* pick_read = L.pick[k];
    unsigned long long* pick = L.pick[k];
    for (;;) {
        // the two smallest keys of the wave (keys are unique): the lane's own pair, then two rounds of ds_min_u64 on one LDS word each — the lanes that hold a
        // live count add theirs, everyone reads the minimum back; the second round leaves the first one's winner out
        unsigned long long m1 = kNoKey, m2 = kNoKey;
        #pragma unroll
        for (int j = 0; j < 5; ++j) {
            const unsigned long long key = freq[j] ? (unsigned long long)freq[j] << 9 | (unsigned long long)(511 - (lane + 64 * j)) : kNoKey;
            if (key < m1) { m2 = m1; m1 = key; } else if (key < m2) m2 = key;
        }
        if (lane == 0) { pick[0] = kNoKey; pick[1] = kNoKey; }
        wave_sync();
        if (m1 != kNoKey) atomicMin(&pick[0], m1);
        wave_sync();
        const unsigned long long g1 = pick_read[0];
        { const unsigned long long mine = m1 == g1 ? m2 : m1; if (mine != kNoKey) atomicMin(&pick[1], mine); }
        wave_sync();
        m1 = g1; m2 = pick_read[1];
        wave_sync();                                        // (both are read before lane 0 resets them)
        if (m2 == kNoKey) break;                            // (wave-uniform)
        const int c1 = 511 - (int)(m1 & 511), c2 = 511 - (int)(m2 & 511);
        const uint32_t f2 = (uint32_t)(m2 >> 9);
        #pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int idx = lane + 64 * j;
            if (tree[j] == c1 || tree[j] == c2) { ++len[j]; tree[j] = c1; }
            if (idx == c1) freq[j] += f2;
            if (idx == c2) freq[j] = 0;
        }
    }
    wave_sync();
    int longest = 0;
    #pragma unroll
    for (int j = 0; j < 5; ++j) {
        if (len[j]) atomicAdd(&L.of_length[k][len[j]], 1u);
        longest = max(longest, len[j]);
        if (j < 4) L.key[k][lane + 64 * j] = len[j] ? (uint32_t)len[j] << 8 | (uint32_t)(lane + 64 * j) : ~0u;
    }
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) longest = max(longest, __shfl_xor(longest, d, 64));
    wave_sync();
    if (lane == 0) {
        uint32_t* bits = L.of_length[k];
        for (int i = longest; i > 16; --i)                  // Annex K.3
            while (bits[i] > 0) {
                int j = i - 2;
                while (j > 0 && bits[j] == 0) --j;
                bits[i] -= 2; bits[i - 1] += 1; bits[j + 1] += 2; bits[j] -= 1;
            }
        int last = 16;
        while (last > 1 && bits[last] == 0) --last;
        if (bits[last]) --bits[last];                       // the reserved entry
        uint32_t code = 0, place = 0;
        out->dht[k][0] = (uint8_t)((k & 1) << 4 | k >> 1);
        for (int l = 1; l <= 16; ++l) {
            L.first_code[k][l] = code; L.first_place[k][l] = place; L.codes[k][l] = bits[l];
            out->dht[k][l] = (uint8_t)bits[l];
            code = (code + bits[l]) << 1; place += bits[l];
        }
        out->n[k] = place;
    }
    wave_sync();
    // a symbol's place among the DHT's values: the number of smaller keys
    uint32_t mine[4], place[4] = {0, 0, 0, 0};
    #pragma unroll
    for (int j = 0; j < 4; ++j) mine[j] = L.key[k][lane + 64 * j];
    for (int i = 0; i < 256; ++i) {
        const uint32_t other = L.key[k][i];
        #pragma unroll
        for (int j = 0; j < 4; ++j) place[j] += other < mine[j];
    }
    uint32_t* entries = k & 1 ? out->huff.ac[k >> 1] : out->huff.dc[k >> 1];
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx = lane + 64 * j;
        if (idx >= n_sym) continue;
        uint32_t entry = 0;
        if (mine[j] != ~0u) {
            for (int l = 1; l <= 16; ++l)
                if (place[j] >= L.first_place[k][l] && place[j] - L.first_place[k][l] < L.codes[k][l]) entry = (L.first_code[k][l] + place[j] - L.first_place[k][l]) << 8 | (uint32_t)l;
            out->dht[k][17 + place[j]] = (uint8_t)idx;
        }
        entries[idx] = entry;
    }
}

namespace {
constexpr int kPackGroup = 8;                               // segments per workgroup
}

// OPT: the header is the fixed one's bytes around the DHT that k_jpeg_tables built (`opt`), 197 + sum(17 + n) bytes, and the data begins behind it
template <bool OPT>
__global__ void __launch_bounds__(256) k_jpeg_pack(const uint8_t* __restrict__ scratch, const uint32_t* __restrict__ lengths, const QualityTables* __restrict__ tables,
                                                   const OptTables* __restrict__ opt, int n_seg, int w, int h, int sof_sampling, int restart, uint8_t* __restrict__ frame,
                                                   uint32_t* __restrict__ total_host, const BudgetSearch* __restrict__ search) {
    constexpr size_t kSlot = OPT ? kJpegOptSlotBytes : kJpegSlotBytes;
    if (search) tables += picked_quality(search) - 1;      // (as in k_jpeg_code: the header's bytes are the picked quality's)
    int dht_bytes[4] = {0, 0, 0, 0}, header_bytes = kHeaderBytes;
    if constexpr (OPT) {
        header_bytes = kOptHeaderFixed;
        for (int k = 0; k < 4; ++k) { dht_bytes[k] = 17 + (int)min(opt->n[k], 256u); header_bytes += dht_bytes[k]; }
    }
    const size_t data = 4 + (size_t)header_bytes;           // the frame's offset of the entropy-coded data (not OPT: kFrameData)
    __shared__ unsigned long long s_part[2][4];
    __shared__ uint32_t s_off[kPackGroup + 1];
    const int t = threadIdx.x, first = blockIdx.x * kPackGroup;
    unsigned long long before = 0, all = 0;
    for (int i = t; i < n_seg; i += 256) { const uint32_t v = lengths[i] + 2; all += v; if (i < first) before += v; }      // (a segment and its marker)
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { before += __shfl_xor(before, d, 64); all += __shfl_xor(all, d, 64); }
    if ((t & 63) == 0) { s_part[0][t >> 6] = before; s_part[1][t >> 6] = all; }
    __syncthreads();
    const size_t base = data + (size_t)(s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3]);
    const size_t total = data + (size_t)(s_part[1][0] + s_part[1][1] + s_part[1][2] + s_part[1][3]);
    if (t == 0) {
        uint32_t o = 0;
        for (int k = 0; k < kPackGroup; ++k) { s_off[k] = o; if (first + k < n_seg) o += lengths[first + k] + 2; }
        s_off[kPackGroup] = o;
    }
    __syncthreads();
    for (int k = 0; k < kPackGroup && first + k < n_seg; ++k) {
        const int seg = first + k;
        const uint8_t* src = scratch + (size_t)seg * kSlot;
        const uint32_t n = s_off[k + 1] - s_off[k] - 2;
        uint8_t* dst = frame + base + s_off[k];
        for (uint32_t j = t; j < n; j += 256) dst[j] = src[j];
        if (t == 0) { dst[n] = 0xFF; dst[n + 1] = seg == n_seg - 1 ? (uint8_t)0xD9 : (uint8_t)(0xD0 + (seg & 7)); }
    }
    if (blockIdx.x == 0) {
        for (int at = t; at < header_bytes; at += 256) {
            int i = at;                                     // the fixed header's byte that stands here
            if constexpr (OPT) if (at >= kOffDht) {
                int j = at - kOffDht - 4, table = 0;        // inside the DHT: its marker and length, then the tables' bytes; behind it DRI and SOS
                const int dht_length = 2 + header_bytes - kOptHeaderFixed;
                if (j < 0) { frame[4 + at] = j == -4 ? (uint8_t)0xFF : j == -3 ? (uint8_t)0xC4 : j == -2 ? (uint8_t)(dht_length >> 8) : (uint8_t)dht_length; continue; }
                while (table < 4 && j >= dht_bytes[table]) j -= dht_bytes[table++];
                if (table < 4) { frame[4 + at] = opt->dht[table][j]; continue; }
                i = kOffDri + j;
            }
            const int k = i - kOffSofHeight;                // SOF0's height and width, big-endian; the two bytes of the sampling: component 1's factors, DRI's interval
            frame[4 + at] = k == 0 ? (uint8_t)(h >> 8) : k == 1 ? (uint8_t)h : k == 2 ? (uint8_t)(w >> 8) : k == 3 ? (uint8_t)w :
                           i == kOffSofSampling ? (uint8_t)sof_sampling : i == kOffDriLow ? (uint8_t)restart : tables->header[i];
        }
        if (t == 0) {
            *(uint32_t*)frame = (uint32_t)total;            // (the frame's buffer comes from hipMalloc: aligned)
            if (total_host) { *total_host = (uint32_t)total; __threadfence_system(); }
        }
    }
}

namespace {
size_t slot_bytes(bool opt) { return opt ? kJpegOptSlotBytes : kJpegSlotBytes; }
uint32_t* jpeg_lengths(uint8_t* scratch, size_t n_seg, bool opt) { return (uint32_t*)(scratch + n_seg * slot_bytes(opt)); }
// the OPT scratch behind the slots and the lengths: the built tables, then the frame's counts
int count_groups(size_t n_seg) { return (int)std::min<size_t>((n_seg + kCountWaves - 1) / kCountWaves, (size_t)kCountGroupsMax); }
OptTables* jpeg_opt_tables(uint8_t* scratch, size_t n_seg) { return (OptTables*)(scratch + ((n_seg * (kJpegOptSlotBytes + 4) + 15) & ~(size_t)15)); }
uint32_t* jpeg_opt_counts(uint8_t* scratch, size_t n_seg) { return (uint32_t*)(jpeg_opt_tables(scratch, n_seg) + 1); }
static_assert(sizeof(OptTables) % 16 == 0 && kJpegOptSlotBytes % 4 == 0, "the scratch's parts are aligned");

// the scratch of the formats on the Annex K tables, behind the slots and the lengths: the budget's search state, then the lengths it measures
BudgetSearch* jpeg_budget_search(uint8_t* scratch, size_t n_seg) { return (BudgetSearch*)(scratch + ((n_seg * (kJpegSlotBytes + 4) + 15) & ~(size_t)15)); }
uint32_t* jpeg_budget_measured(uint8_t* scratch, size_t n_seg) { return (uint32_t*)(jpeg_budget_search(scratch, n_seg) + 1); }
static_assert(sizeof(BudgetSearch) == 16 && sizeof(QualityTables) % 4 == 0, "the scratch's parts and the 100 tables are aligned");
}

size_t jpeg_scratch_bytes(int w, int h, Sampling sm, bool opt) {
    const size_t n_seg = segment_count((size_t)w, (size_t)h, sm);
    if (!opt) return ((n_seg * (kJpegSlotBytes + 4) + 15) & ~(size_t)15) + sizeof(BudgetSearch) + n_seg * 4 * kBudgetListMax + 16;
    return ((n_seg * (kJpegOptSlotBytes + 4) + 15) & ~(size_t)15) + sizeof(OptTables) + sizeof(SymbolCounts) + 16;
}

void launch_jpeg_count_into(const uint8_t* planes, const void* tables, uint32_t* counts, int w, int h, Sampling sm, hipStream_t s, hipEvent_t done) {
    const size_t n_seg = segment_count((size_t)w, (size_t)h, sm);
    const int mw = (w + mcu_side(sm) - 1) / mcu_side(sm);
    auto kernel = sm == k444 ? k_jpeg_count<k444> : k_jpeg_count<k420>;
    const dim3 grid((unsigned)count_groups(n_seg)), block(64 * kCountWaves);
    const int n_mcu = (int)mcu_count((size_t)w, (size_t)h, sm);
    if (done) hipExtLaunchKernelGGL(kernel, grid, block, 0, s, nullptr, done, 0, planes, (const QualityTables*)tables, counts, w, h, mw, n_mcu, (int)n_seg);
    else hipLaunchKernelGGL(kernel, grid, block, 0, s, planes, (const QualityTables*)tables, counts, w, h, mw, n_mcu, (int)n_seg);
}
void launch_jpeg_count(const uint8_t* planes, const void* tables, uint8_t* scratch, int w, int h, Sampling sm, hipStream_t s) {
    launch_jpeg_count_into(planes, tables, jpeg_opt_counts(scratch, segment_count((size_t)w, (size_t)h, sm)), w, h, sm, s, nullptr);
}

void launch_jpeg_table_build(uint32_t* counts, void* built, hipStream_t s) {
    hipLaunchKernelGGL(k_jpeg_tables, dim3(1), dim3(256), 0, s, counts, (OptTables*)built);
}
void launch_jpeg_tables(uint8_t* scratch, int w, int h, Sampling sm, hipStream_t s) {
    const size_t n_seg = segment_count((size_t)w, (size_t)h, sm);
    launch_jpeg_table_build(jpeg_opt_counts(scratch, n_seg), jpeg_opt_tables(scratch, n_seg), s);
}

hipError_t launch_jpeg_counts_clear(uint8_t* scratch, int w, int h, Sampling sm, hipStream_t s) {
    return hipMemsetAsync(jpeg_opt_counts(scratch, segment_count((size_t)w, (size_t)h, sm)), 0, sizeof(SymbolCounts), s);
}

// built: null for the Annex K tables, or the OptTables that a table build left — the scratch's own (launch_jpeg_code) or a sequence's (launch_jpeg_code_on)
static void launch_jpeg_code_with(const uint8_t* planes, const void* tables, const void* built, const BudgetSearch* search, uint8_t* scratch, int w, int h, Sampling sm, hipStream_t s) {
    const size_t n_seg = segment_count((size_t)w, (size_t)h, sm);
    const int mw = (w + mcu_side(sm) - 1) / mcu_side(sm);
    const bool opt = built != nullptr;
    auto kernel = opt ? (sm == k444 ? k_jpeg_code<k444, true> : k_jpeg_code<k420, true>) : (sm == k444 ? k_jpeg_code<k444, false> : k_jpeg_code<k420, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_seg), dim3(64), 0, s, planes, (const QualityTables*)tables, opt ? &((const OptTables*)built)->huff : (const HuffTables*)nullptr,
                       scratch, jpeg_lengths(scratch, n_seg, opt), w, h, mw, (int)mcu_count((size_t)w, (size_t)h, sm), search);
}
void launch_jpeg_code_on(const uint8_t* planes, const void* tables, const void* built, uint8_t* scratch, int w, int h, Sampling sm, hipStream_t s) {
    launch_jpeg_code_with(planes, tables, built, nullptr, scratch, w, h, sm, s);
}
void launch_jpeg_code(const uint8_t* planes, const void* tables, uint8_t* scratch, int w, int h, Sampling sm, bool opt, hipStream_t s) {
    launch_jpeg_code_on(planes, tables, opt ? jpeg_opt_tables(scratch, segment_count((size_t)w, (size_t)h, sm)) : nullptr, scratch, w, h, sm, s);
}

static void launch_jpeg_pack_with(const void* tables, const void* built, const BudgetSearch* search, const uint8_t* scratch, uint8_t* frame, uint32_t* total_host, int w, int h, Sampling sm, hipStream_t s, hipEvent_t done) {
    const size_t n_seg = segment_count((size_t)w, (size_t)h, sm);
    const bool opt = built != nullptr;
    hipExtLaunchKernelGGL(opt ? k_jpeg_pack<true> : k_jpeg_pack<false>, dim3((unsigned)((n_seg + kPackGroup - 1) / kPackGroup)), dim3(256), 0, s, nullptr, done, 0, scratch,
                          jpeg_lengths(const_cast<uint8_t*>(scratch), n_seg, opt), (const QualityTables*)tables, (const OptTables*)built, (int)n_seg, w, h,
                          (int)sof_sampling(sm), restart_mcus(sm), frame, total_host, search);
}
void launch_jpeg_pack_on(const void* tables, const void* built, const uint8_t* scratch, uint8_t* frame, uint32_t* total_host, int w, int h, Sampling sm, hipStream_t s, hipEvent_t done) {
    launch_jpeg_pack_with(tables, built, nullptr, scratch, frame, total_host, w, h, sm, s, done);
}
void launch_jpeg_pack(const void* tables, const uint8_t* scratch, uint8_t* frame, uint32_t* total_host, int w, int h, Sampling sm, bool opt, hipStream_t s, hipEvent_t done) {
    launch_jpeg_pack_on(tables, opt ? jpeg_opt_tables(const_cast<uint8_t*>(scratch), segment_count((size_t)w, (size_t)h, sm)) : nullptr, scratch, frame, total_host, w, h, sm, s, done);
}

// ---- the byte budget: steps of one measuring and one picking dispatch each, then the coder and the gather on the picked quality's tables ----
void launch_jpeg_measure(const uint8_t* planes, const JpegBudget& budget, uint8_t* scratch, int step, int w, int h, Sampling sm, hipStream_t s) {
    const size_t n_seg = segment_count((size_t)w, (size_t)h, sm);
    const int mw = (w + mcu_side(sm) - 1) / mcu_side(sm);
    hipLaunchKernelGGL(sm == k444 ? k_jpeg_measure<k444> : k_jpeg_measure<k420>, dim3((unsigned)n_seg), dim3(64), 0, s, planes, (const QualityTables*)budget.tables,
                       (const JpegBudgetParams*)budget.params, (const BudgetSearch*)jpeg_budget_search(scratch, n_seg), jpeg_budget_measured(scratch, n_seg), (int)(step == 0), w, h, mw,
                       (int)mcu_count((size_t)w, (size_t)h, sm), (int)n_seg, (size_t)0, 0, 1);
}
void launch_jpeg_pick(const JpegBudget& budget, uint8_t* scratch, int step, int w, int h, Sampling sm, hipStream_t s) {
    const size_t n_seg = segment_count((size_t)w, (size_t)h, sm);
    hipLaunchKernelGGL(k_jpeg_pick<false>, dim3(1), dim3(256), 0, s, (const JpegBudgetParams*)budget.params, jpeg_budget_search(scratch, n_seg), (const uint32_t*)jpeg_budget_measured(scratch, n_seg),
                       (int)(step == 0), (int)n_seg, 1);
}
// (the picked quality is read from `state`: the frame's own search state in its scratch, or a sequence's)
void launch_jpeg_code_picked_by(const uint8_t* planes, const JpegBudget& budget, const uint8_t* state, uint8_t* scratch, int w, int h, Sampling sm, hipStream_t s) {
    launch_jpeg_code_with(planes, budget.tables, nullptr, (const BudgetSearch*)state, scratch, w, h, sm, s);
}
void launch_jpeg_pack_picked_by(const JpegBudget& budget, const uint8_t* state, const uint8_t* scratch, uint8_t* frame, uint32_t* total_host, int w, int h, Sampling sm, hipStream_t s, hipEvent_t done) {
    launch_jpeg_pack_with(budget.tables, nullptr, (const BudgetSearch*)state, scratch, frame, total_host, w, h, sm, s, done);
}
void launch_jpeg_code_picked(const uint8_t* planes, const JpegBudget& budget, uint8_t* scratch, int w, int h, Sampling sm, hipStream_t s) {
    launch_jpeg_code_picked_by(planes, budget, (const uint8_t*)jpeg_budget_search(scratch, segment_count((size_t)w, (size_t)h, sm)), scratch, w, h, sm, s);
}
void launch_jpeg_pack_picked(const JpegBudget& budget, const uint8_t* scratch, uint8_t* frame, uint32_t* total_host, int w, int h, Sampling sm, hipStream_t s, hipEvent_t done) {
    launch_jpeg_pack_picked_by(budget, (const uint8_t*)jpeg_budget_search(const_cast<uint8_t*>(scratch), segment_count((size_t)w, (size_t)h, sm)), scratch, frame, total_host, w, h, sm, s, done);
}

// ---- the sequence budget: the same steps once for all the frames of a store, the search's state and the measured lengths in `state` (jpeg_seq_budget_bytes) ----
static_assert(offsetof(JpegSeqBudgetParams, quality_max) == offsetof(JpegBudgetParams, quality_max) && sizeof(JpegSeqBudgetParams) == 16, "search_state reads the highest quality from either");
namespace {
constexpr int kSeqMeasureFrames = 32768;                    // frames of one measuring launch (a grid's second dimension ends at 65535): a longer sequence takes several per step
}
size_t jpeg_seq_budget_bytes(int n_frames, int w, int h, Sampling sm) {
    return sizeof(BudgetSearch) + (size_t)n_frames * segment_count((size_t)w, (size_t)h, sm) * 4 * kBudgetListMax + 16;
}
void launch_jpeg_seq_measure(const uint8_t* store, size_t frame_stride, int n_frames, const JpegBudget& budget, uint8_t* state, int step, int w, int h, Sampling sm, hipStream_t s) {
    const size_t n_seg = segment_count((size_t)w, (size_t)h, sm);
    const int mw = (w + mcu_side(sm) - 1) / mcu_side(sm);
    for (int frame0 = 0; frame0 < n_frames; frame0 += kSeqMeasureFrames)
        hipLaunchKernelGGL(sm == k444 ? k_jpeg_measure<k444> : k_jpeg_measure<k420>, dim3((unsigned)n_seg, (unsigned)std::min(kSeqMeasureFrames, n_frames - frame0)), dim3(64), 0, s, store,
                           (const QualityTables*)budget.tables, (const JpegBudgetParams*)budget.params, (const BudgetSearch*)state, (uint32_t*)(state + sizeof(BudgetSearch)), (int)(step == 0), w, h, mw,
                           (int)mcu_count((size_t)w, (size_t)h, sm), (int)n_seg, frame_stride, frame0, n_frames);
}
void launch_jpeg_seq_pick(const JpegBudget& budget, uint8_t* state, int n_frames, int step, int w, int h, Sampling sm, hipStream_t s) {
    hipLaunchKernelGGL(k_jpeg_pick<true>, dim3(1), dim3(256), 0, s, (const JpegBudgetParams*)budget.params, (BudgetSearch*)state, (const uint32_t*)(state + sizeof(BudgetSearch)),
                       (int)(step == 0), (int)segment_count((size_t)w, (size_t)h, sm), n_frames);
}

}  // namespace poppy_hip
