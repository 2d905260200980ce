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
#include "kernels.h"
#include <hip/hip_ext.h>
#include <utility>

namespace poppy_hip {

namespace {

using namespace jpeg;

constexpr int kSegLanes = 6 * kRestartMcus;                 // blocks of a full segment
static_assert(kSegLanes <= 64, "a segment's blocks are the lanes of one wave");
static_assert(mcu_blocks(k444) * kRestartMcus444 == kSegLanes, "... of either sampling: the bit buffer and the scratch slot below are sized for them");
constexpr int kBitWords = (int)((6 * kBlockBitsMax * kRestartMcus + 31) / 32) + 2;      // the segment's bits at their bound, the word a code may spill into
static_assert(kJpegSlotBytes >= 2 * ((6 * kBlockBitsMax * kRestartMcus + 7) / 8), "a slot holds a segment with every byte stuffed");

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

struct CoderLds {
    int16_t coef[64][64];                                   // [zig-zag position][lane]
    uint32_t bits[kBitWords];                               // the segment's bit string, most significant bit of word 0 first
    uint32_t ac[2][256];
    uint32_t dc[2][16];
    uint2 q[2][64];                                         // per table and natural index: the bias 4 Q, the reciprocal of 8 Q
};

// coefficient N of the lane's block: quantised, into its zig-zag row; returns it
template <int N>
__device__ __forceinline__ int quantise_store(CoderLds& L, int F, int table, int lane) {
    constexpr int pos = zigzag_position(N);
    const uint2 q = L.q[table][N];
    const uint32_t a = (uint32_t)(F < 0 ? -F : F);
    const int m = (int)__umulhi(a + q.x, q.y);
    const int v = F < 0 ? -m : m;
    L.coef[pos][lane] = (int16_t)v;
    return v;
}
template <int... N>
__device__ __forceinline__ int quantise_block(CoderLds& L, const int (&f)[64], int table, int lane, std::integer_sequence<int, N...>) {
    int dc = 0;
    ((N == 0 ? (void)(dc = quantise_store<N>(L, f[N], table, lane)) : (void)quantise_store<N>(L, f[N], table, lane)), ...);
    return dc;
}

// `len` bits (1..26), right-aligned in `value`, at bit position `at` of the segment
__device__ __forceinline__ void emit_bits(uint32_t* bits, uint32_t at, uint32_t value, int len) {
    const uint32_t word = at >> 5, off = at & 31;
    const unsigned long long x = (unsigned long long)value << (64 - (int)off - len);
    atomicOr(&bits[word], (uint32_t)(x >> 32));
    if (off + (uint32_t)len > 32) atomicOr(&bits[word + 1], (uint32_t)x);
}

__device__ __forceinline__ int category(int v) { return 32 - __clz(v < 0 ? -v : v); }      // (__clz(0) is 32)

// The lane's block as Huffman codes: counted (EMIT false) or ORed into the bit buffer from position `at` on.  Returns the block's bits.
template <bool EMIT>
__device__ __forceinline__ uint32_t code_block(CoderLds& L, int lane, int table, int diff, uint32_t at) {
    uint32_t n = 0;
    auto put = [&](uint32_t huff, int v, int cat) {          // a symbol's code, then the value's low `cat` bits
        const int len = (int)(huff & 255) + cat;
        if (EMIT) emit_bits(L.bits, at + n, (huff >> 8) << cat | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1)), len);
        n += (uint32_t)len;
    };
    { const int cat = category(diff); put(L.dc[table][cat], diff, cat); }
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = L.coef[k][lane];
        if (v == 0) { ++run; continue; }
        for (; run >= 16; run -= 16) put(L.ac[table][0xF0], 0, 0);
        const int cat = category(v);
        put(L.ac[table][run << 4 | cat], v, cat);
        run = 0;
    }
    if (run) put(L.ac[table][0], 0, 0);
    return n;
}

}  // namespace

template <Sampling S>
__global__ void __launch_bounds__(64) k_jpeg_code(const uint8_t* __restrict__ i420, const QualityTables* __restrict__ tables, uint8_t* __restrict__ scratch,
                                                  uint32_t* __restrict__ lengths, int w, int h, int mw, int n_mcu) {
    constexpr int kBlocks = mcu_blocks(S), kMcus = restart_mcus(S);
    __shared__ CoderLds L;
    const int lane = threadIdx.x, seg = blockIdx.x;
    for (int i = lane; i < 512; i += 64) L.ac[i >> 8][i & 255] = c_huff.ac[i >> 8][i & 255];
    if (lane < 32) L.dc[lane >> 4][lane & 15] = c_huff.dc[lane >> 4][lane & 15];
    for (int i = lane; i < 128; i += 64) L.q[i >> 6][i & 63] = make_uint2(tables->bias[i >> 6][i & 63], tables->recip[i >> 6][i & 63]);
    wave_sync();
    const int first = seg * kMcus, mcus = min(kMcus, n_mcu - first);
    const int m_in = lane / kBlocks, b = lane - kBlocks * m_in, table = S == k444 ? b >= 1 : b >= 4;
    const bool active = m_in < mcus;
    int dc = 0;
    if (active) {
        const int m = first + m_in, my = m / mw, mx = m - my * mw;
        // the block's plane, that plane's size and the block's origin in it.  4:4:4: (the I444 planes) every plane w x h, every block at (8 mx, 8 my)
        const int cw = S == k444 ? w : (w + 1) / 2, ch = S == k444 ? h : (h + 1) / 2;
        const int pw = table ? cw : w, ph = table ? ch : h;
        const int x0 = table || S == k444 ? 8 * mx : 16 * mx + 8 * (b & 1), y0 = table || S == k444 ? 8 * my : 16 * my + 8 * (b >> 1);
        const uint8_t* plane = i420 + (!table ? (size_t)0 : (size_t)w * h + (b == kBlocks - 1 ? (size_t)cw * ch : (size_t)0));
        int f[64];
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
        dc = quantise_block(L, f, table, lane, std::make_integer_sequence<int, 64>());
    }
    // the previous block of the same component: the luma block before, Y11 of the MCU before for Y00, the same chroma block of the MCU before; the segment's first: 0
    // (4:4:4: the same block of the MCU before, three lanes down)
    const int from = S == k444 ? lane - 3 : b >= 4 ? lane - 6 : b == 0 ? lane - 3 : lane - 1;
    const int before = __shfl(dc, max(from, 0), 64);
    const int diff = dc - ((S == k444 || b == 0 || b >= 4) && m_in == 0 ? 0 : before);
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
    // byte stuffing: byte i of the string goes to i + (the FF bytes in front of it), a zero byte behind every FF
    const uint32_t n_bytes = (total_bits + 7) / 8;
    uint8_t* dst = scratch + (size_t)seg * kJpegSlotBytes;
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

namespace {
constexpr int kPackGroup = 8;                               // segments per workgroup
}

__global__ void __launch_bounds__(256) k_jpeg_pack(const uint8_t* __restrict__ scratch, const uint32_t* __restrict__ lengths, const QualityTables* __restrict__ tables,
                                                   int n_seg, int w, int h, int sof_sampling, int restart, uint8_t* __restrict__ frame, uint32_t* __restrict__ total_host) {
    __shared__ unsigned long long s_part[2][4];
    __shared__ uint32_t s_off[kPackGroup + 1];
    const int t = threadIdx.x, first = blockIdx.x * kPackGroup;
    unsigned long long before = 0, all = 0;
    for (int i = t; i < n_seg; i += 256) { const uint32_t v = lengths[i] + 2; all += v; if (i < first) before += v; }      // (a segment and its marker)
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { before += __shfl_xor(before, d, 64); all += __shfl_xor(all, d, 64); }
    if ((t & 63) == 0) { s_part[0][t >> 6] = before; s_part[1][t >> 6] = all; }
    __syncthreads();
    const size_t base = kFrameData + (size_t)(s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3]);
    const size_t total = kFrameData + (size_t)(s_part[1][0] + s_part[1][1] + s_part[1][2] + s_part[1][3]);
    if (t == 0) {
        uint32_t o = 0;
        for (int k = 0; k < kPackGroup; ++k) { s_off[k] = o; if (first + k < n_seg) o += lengths[first + k] + 2; }
        s_off[kPackGroup] = o;
    }
    __syncthreads();
    for (int k = 0; k < kPackGroup && first + k < n_seg; ++k) {
        const int seg = first + k;
        const uint8_t* src = scratch + (size_t)seg * kJpegSlotBytes;
        const uint32_t n = s_off[k + 1] - s_off[k] - 2;
        uint8_t* dst = frame + base + s_off[k];
        for (uint32_t j = t; j < n; j += 256) dst[j] = src[j];
        if (t == 0) { dst[n] = 0xFF; dst[n + 1] = seg == n_seg - 1 ? (uint8_t)0xD9 : (uint8_t)(0xD0 + (seg & 7)); }
    }
    if (blockIdx.x == 0) {
        for (int i = t; i < kHeaderBytes; i += 256) {
            const int k = i - kOffSofHeight;                // SOF0's height and width, big-endian; the two bytes of the sampling: component 1's factors, DRI's interval
            frame[4 + i] = k == 0 ? (uint8_t)(h >> 8) : k == 1 ? (uint8_t)h : k == 2 ? (uint8_t)(w >> 8) : k == 3 ? (uint8_t)w :
                           i == kOffSofSampling ? (uint8_t)sof_sampling : i == kOffDriLow ? (uint8_t)restart : tables->header[i];
        }
        if (t == 0) {
            *(uint32_t*)frame = (uint32_t)total;            // (the frame's buffer comes from hipMalloc: aligned)
            if (total_host) { *total_host = (uint32_t)total; __threadfence_system(); }
        }
    }
}

namespace {
uint32_t* jpeg_lengths(uint8_t* scratch, size_t n_seg) { return (uint32_t*)(scratch + n_seg * kJpegSlotBytes); }
}

size_t jpeg_scratch_bytes(int w, int h, Sampling sm) { return segment_count((size_t)w, (size_t)h, sm) * (kJpegSlotBytes + 4) + 16; }

void launch_jpeg_code(const uint8_t* planes, const void* tables, uint8_t* scratch, int w, int h, Sampling sm, hipStream_t s) {
    const size_t n_seg = segment_count((size_t)w, (size_t)h, sm);
    const int mw = (w + mcu_side(sm) - 1) / mcu_side(sm);
    hipLaunchKernelGGL(sm == k444 ? k_jpeg_code<k444> : k_jpeg_code<k420>, dim3((unsigned)n_seg), dim3(64), 0, s, planes, (const QualityTables*)tables, scratch,
                       jpeg_lengths(scratch, n_seg), w, h, mw, (int)mcu_count((size_t)w, (size_t)h, sm));
}

void launch_jpeg_pack(const void* tables, const uint8_t* scratch, uint8_t* frame, uint32_t* total_host, int w, int h, Sampling sm, hipStream_t s, hipEvent_t done) {
    const size_t n_seg = segment_count((size_t)w, (size_t)h, sm);
    hipExtLaunchKernelGGL(k_jpeg_pack, dim3((unsigned)((n_seg + kPackGroup - 1) / kPackGroup)), dim3(256), 0, s, nullptr, done, 0, scratch,
                          jpeg_lengths(const_cast<uint8_t*>(scratch), n_seg), (const QualityTables*)tables, (int)n_seg, w, h, (int)sof_sampling(sm), restart_mcus(sm), frame,
                          total_host);
}

}  // namespace poppy_hip
