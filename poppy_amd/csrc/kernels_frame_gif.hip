// kernels_frame_gif.hip — a PAL8 frame on the device (index plane + palette: kernels_frame_pal8.hip) -> POPPY_FRAME_GIF for the writer hand-off (include/poppy_hip.h):
// the index plane LZW-coded in independent segments of POPPY_GIF_SEGMENT_PIXELS pixels and framed as GIF image data.  poppy_pal8_to_gif_frame (frame_gif.cpp) is the
// host statement; the bytes are equal.
//
// Two dispatches behind k_pal8_remap, no host round trip:
//   k_gif_lzw    a segment per wave, kLzwWaves waves per workgroup, every wave on LDS of its own (no workgroup barrier).  All lanes stage the segment's index bytes and
//                clear the hash table; lane 0 then runs the match loop, which is the kernel's time: the loop is serial by nature, the parallelism is across the
//                segments (1013 at 1080p with 2048 pixels each, four per compute unit, all resident at once).  Measured ≈ 580 cycles per pixel (493 us per 1080p frame,
//                DESIGN.md section 4), ten times the dependent LDS look-up's ≈ 50: the suspected cause is that the loop runs on ONE lane under an execution mask — every
//                branch is a mask save / restore around vector instructions issued at the vector rate, the 64-bit accumulator shifts are several instructions each.  The table is open
//                addressing over key = prefix << 8 | byte, an entry is key << 12 | code (0xffffffff: free; no entry has that value, a string with prefix 4095 is never
//                added), 2 S entries for a segment of S pixels (at most S - 1 strings live).  The codes go through a 64-bit accumulator into an LDS bit buffer, 32 bits
//                at a time.  A full table (possible from 3839 pixels on) ends lane 0's run, all lanes clear the table, lane 0 goes on.  At the end all lanes store the
//                segment's bytes into its fixed slot (kGifSlotBytes apart) of the scratch buffer, and lane 0 the byte length.
//   k_gif_pack   every workgroup sums the lengths in front of its group of segments (at most 16 384 words: a sum inside the kernel, no scan kernel) and all of them for
//                the payload's length, then moves its segments' bytes to their place in the frame with the sub-block framing applied on the fly: payload byte i goes to
//                773 + i + i / 255 + 1, the thread that stores the first byte of a sub-block also stores the length byte in front of it.  Workgroup 0 writes the
//                minimum-code-size byte, the terminator, the palette and `total` — into the frame and into a word of mapped pinned host memory, so that the host knows
//                how many bytes to copy when the frame's completion event has fired, without a copy packet of its own in the stream.
//
// POPPY_FRAME_GIF_SEQ (one palette per sequence, poppy_bgr_frames_to_gif_frames is its host statement) codes from the sequence store instead:
//   k_gif_lzw_bgr  k_gif_lzw with another staging (gif_lzw_segment is the code of both): the lanes read the segment's BGR from the frame's place in the store, look every
//                pixel's cell up in the sequence's 32 KiB cell -> index table in global memory and write the index bytes into the wave's s_px, so k_pal8_remap's
//                dispatch and the index plane in HBM fall away.  The table is not copied to LDS: 32 KiB more per workgroup would leave one workgroup per compute
//                unit where three run now.
//   k_gif_pack   as it is, with the palette read from the sequence's tables.
#include "kernels.h"
#include "pal8_cells.h"
#include <hip/hip_ext.h>

namespace poppy_hip {

namespace {

constexpr int kSeg = POPPY_GIF_SEGMENT_PIXELS;
static_assert(kSeg == 1024 || kSeg == 2048 || kSeg == 4096, "POPPY_GIF_SEGMENT_PIXELS is 1024, 2048 or 4096");
constexpr int kTable = 2 * kSeg;                            // entries; a power of two
constexpr int kTableBits = kSeg == 1024 ? 11 : kSeg == 2048 ? 12 : 13;
constexpr int kOutWords = (int)(kGifSlotBytes / 4);
constexpr int kLzwWaves = 4096 / kSeg;                      // 4, 2, 1: (kSeg + 4 * kTable + kGifSlotBytes) * kLzwWaves is 42 - 43 KiB per workgroup, three workgroups per compute unit
constexpr int kClear = 256, kEnd = 257;

// lanes of one wave run in lockstep: what one lane wrote to LDS is there for the others once the wave's LDS operations have completed and the compiler keeps the order
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

struct BitOut {
    unsigned long long acc = 0;
    int n_acc = 0, n_words = 0;
    __device__ __forceinline__ void put(uint32_t* out, int code, int width) {
        acc |= (unsigned long long)code << n_acc; n_acc += width;
        if (n_acc >= 32) { out[n_words++] = (uint32_t)acc; acc >>= 32; n_acc -= 32; }
    }
};

}  // namespace

namespace {

// The segment's index bytes into the wave's s_px, all lanes; the two stagings are the only difference between k_gif_lzw and k_gif_lzw_bgr.
// From a PAL8 index plane: coalesced; the plane's start is 4-byte aligned (a hipMalloc'd buffer) and kSeg is a multiple of 4, so whole words are read up to the
// plane's last, partial one.
struct StageIndices {
    const uint8_t* __restrict__ idx;
    __device__ __forceinline__ void operator()(uint32_t* px, int at, int len, int lane) const {
        for (int w = lane; w * 4 < len; w += 64) {
            uint32_t v;
            if (w * 4 + 4 <= len) v = *(const uint32_t*)(idx + at + w * 4);
            else { v = 0; for (int k = 0; w * 4 + k < len; ++k) v |= (uint32_t)idx[at + w * 4 + k] << (8 * k); }
            px[w] = v;
        }
    }
};
// From the frame's BGR in the sequence store, through the sequence's cell -> index table (k_pal8_remap's indexing): four pixels = three words per lane and step.  The
// frame's place begins on a 16-byte boundary and a segment on a multiple of kSeg * 3 bytes behind it, so the words are aligned; the frame's last quad, of 1 to 3
// pixels, is read bytewise and never past its last pixel (the place's padding ends before a whole quad would).  The table is read from global memory: 32 KiB that
// every wave of the device touches stay in L2.
struct StageBgr {
    const uint8_t* __restrict__ bgr;
    const uint8_t* __restrict__ table;
    __device__ __forceinline__ void operator()(uint32_t* px, int at, int len, int lane) const {
        const uint8_t* src = bgr + (size_t)at * 3;
        for (int w = lane; w * 4 < len; w += 64) {
            const int n = min(4, len - w * 4);
            uint32_t q[3];
            load_quad(src, (size_t)w, n, true, q);
            uint32_t v = 0;
            #pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) v |= (uint32_t)table[cell_of(quad_byte(q, 3 * k), quad_byte(q, 3 * k + 1), quad_byte(q, 3 * k + 2))] << (8 * k);
            px[w] = v;
        }
    }
};

// One wave's segment: staged by `stage`, coded by lane 0, stored by all lanes (the header comment has the arrangement).
template <typename Stage>
__device__ __forceinline__ void gif_lzw_segment(const Stage stage, uint32_t* __restrict__ scratch, uint32_t* __restrict__ lengths, int n_px, int n_seg) {
    __shared__ uint32_t s_px[kLzwWaves][kSeg / 4];
    __shared__ uint32_t s_tab[kLzwWaves][kTable];
    __shared__ uint32_t s_out[kLzwWaves][kOutWords];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int seg = blockIdx.x * kLzwWaves + wv;
    if (seg >= n_seg) return;                               // (wave-uniform; the kernel has no workgroup barrier)
    const int at = seg * kSeg, len = min(kSeg, n_px - at);
    const bool last = seg == n_seg - 1;
    uint32_t* px = s_px[wv];
    uint32_t* tab = s_tab[wv];
    uint32_t* out = s_out[wv];
    stage(px, at, len, lane);
    for (int i = lane; i < kTable; i += 64) tab[i] = 0xffffffffu;
    wave_sync();
    // lane 0's state lives in its registers across the table restarts
    BitOut bits;
    int width = 9, next = 258, i = 1, prefix = 0;
    bool finished = false;
    if (lane == 0) { bits.put(out, kClear, 9); prefix = (int)(px[0] & 0xffu); }
    for (;;) {
        int restart = 0;
        if (lane == 0) {
            uint32_t word = i < len ? px[i >> 2] : 0u;
            for (; i < len; ++i) {
                if ((i & 3) == 0) word = px[i >> 2];
                const uint32_t byte = (word >> (8 * (i & 3))) & 0xffu;
                const uint32_t key = ((uint32_t)prefix << 8) | byte;
                uint32_t h = (key * 2654435761u) >> (32 - kTableBits);
                uint32_t e = tab[h];
                while (e != 0xffffffffu && (e >> 12) != key) { h = (h + 1) & (kTable - 1); e = tab[h]; }
                if (e != 0xffffffffu) { prefix = (int)(e & 0xfffu); continue; }
                bits.put(out, prefix, width);
                prefix = (int)byte;
                if (next == 4096) { bits.put(out, kClear, width); width = 9; next = 258; restart = 1; ++i; break; }
                tab[h] = (key << 12) | (uint32_t)next;
                if (next == (1 << width)) ++width;
                ++next;
            }
            if (!restart) finished = true;
        }
        restart = __builtin_amdgcn_readfirstlane(restart);
        if (!restart) break;
        wave_sync();
        for (int k = lane; k < kTable; k += 64) tab[k] = 0xffffffffu;
        wave_sync();
    }
    int n_bytes = 0;
    if (lane == 0 && finished) {
        bits.put(out, prefix, width);
        if (last) bits.put(out, kEnd, width);               // ... padded with zero bits to a byte
        else {
            bits.put(out, kClear, width);
            while (bits.n_acc & 7) bits.put(out, kClear, 9);
        }
        n_bytes = bits.n_words * 4 + (bits.n_acc + 7) / 8;
        if (bits.n_acc) out[bits.n_words] = (uint32_t)bits.acc;      // (n_acc < 32: one more word holds the rest)
        lengths[seg] = (uint32_t)n_bytes;
    }
    n_bytes = __builtin_amdgcn_readfirstlane(n_bytes);
    wave_sync();
    uint32_t* dst = scratch + (size_t)seg * kOutWords;
    for (int w = lane; w * 4 < n_bytes && w < kOutWords; w += 64) dst[w] = out[w];
}

}  // namespace

__global__ void __launch_bounds__(64 * kLzwWaves) k_gif_lzw(const uint8_t* __restrict__ idx, uint32_t* __restrict__ scratch, uint32_t* __restrict__ lengths, int n_px, int n_seg) {
    gif_lzw_segment(StageIndices{idx}, scratch, lengths, n_px, n_seg);
}

// bgr: the frame's place in the sequence store (16-byte aligned, tight u8x3); table: the sequence's cell -> index table (32768 bytes)
__global__ void __launch_bounds__(64 * kLzwWaves) k_gif_lzw_bgr(const uint8_t* __restrict__ bgr, const uint8_t* __restrict__ table, uint32_t* __restrict__ scratch,
                                                               uint32_t* __restrict__ lengths, int n_px, int n_seg) {
    gif_lzw_segment(StageBgr{bgr, table}, scratch, lengths, n_px, n_seg);
}

namespace {
constexpr int kPackGroup = 8;                               // segments per workgroup
constexpr size_t kGifData = 773;                            // the frame's offset of the first sub-block's length byte
}

__global__ void __launch_bounds__(256) k_gif_pack(const uint8_t* __restrict__ scratch, const uint32_t* __restrict__ lengths, const uint8_t* __restrict__ palette, int n_seg,
                                                  uint8_t* __restrict__ frame, uint32_t* __restrict__ total_host) {
    __shared__ unsigned long long s_part[2][4];
    __shared__ uint32_t s_off[kPackGroup + 1];
    const int t = threadIdx.x, first = blockIdx.x * kPackGroup;
    unsigned long long before = 0, all = 0;
    for (int i = t; i < n_seg; i += 256) { const uint32_t v = lengths[i]; all += v; if (i < first) before += v; }
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { before += __shfl_xor(before, d, 64); all += __shfl_xor(all, d, 64); }
    if ((t & 63) == 0) { s_part[0][t >> 6] = before; s_part[1][t >> 6] = all; }
    __syncthreads();
    const size_t base = (size_t)(s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3]);
    const size_t payload = (size_t)(s_part[1][0] + s_part[1][1] + s_part[1][2] + s_part[1][3]);
    if (t == 0) {
        uint32_t o = 0;
        for (int k = 0; k < kPackGroup; ++k) { s_off[k] = o; if (first + k < n_seg) o += lengths[first + k]; }
        s_off[kPackGroup] = o;
    }
    __syncthreads();
    for (int k = 0; k < kPackGroup && first + k < n_seg; ++k) {
        const uint8_t* src = scratch + (size_t)(first + k) * kGifSlotBytes;
        const uint32_t n = s_off[k + 1] - s_off[k];
        for (uint32_t j = t; j < n; j += 256) {
            const size_t i = base + s_off[k] + j, block = i / 255;
            if (i - block * 255 == 0) frame[kGifData + block * 256] = (uint8_t)(payload - i >= 255 ? 255 : payload - i);
            frame[kGifData + i + block + 1] = src[j];
        }
    }
    if (blockIdx.x == 0) {
        const size_t end = kGifData + payload + (payload + 254) / 255, total = end + 1;
        for (int i = t; i < 768; i += 256) frame[4 + i] = palette[i];
        if (t == 0) {
            frame[772] = 8;
            frame[end] = 0;
            *(uint32_t*)frame = (uint32_t)total;            // (the frame's buffer comes from hipMalloc: aligned)
            if (total_host) { *total_host = (uint32_t)total; __threadfence_system(); }
        }
    }
}

namespace {
int gif_segments(int w, int h) { return (int)(((size_t)w * h + kSeg - 1) / kSeg); }
uint32_t* gif_lengths(uint8_t* scratch, int n_seg) { return (uint32_t*)(scratch + (size_t)n_seg * kGifSlotBytes); }
void gif_pack(const uint8_t* palette, const uint8_t* scratch, uint8_t* frame, uint32_t* total_host, int n_seg, hipStream_t s, hipEvent_t done) {
    hipExtLaunchKernelGGL(k_gif_pack, dim3((unsigned)((n_seg + kPackGroup - 1) / kPackGroup)), dim3(256), 0, s, nullptr, done, 0, scratch,
                          gif_lengths(const_cast<uint8_t*>(scratch), n_seg), palette, n_seg, frame, total_host);
}
}  // namespace

void launch_gif_lzw(const uint8_t* pal8, uint8_t* scratch, int w, int h, hipStream_t s) {
    const int n_seg = gif_segments(w, h);
    hipLaunchKernelGGL(k_gif_lzw, dim3((unsigned)((n_seg + kLzwWaves - 1) / kLzwWaves)), dim3(64 * kLzwWaves), 0, s, pal8, (uint32_t*)scratch, gif_lengths(scratch, n_seg), (int)((size_t)w * h), n_seg);
}

void launch_gif_pack(const uint8_t* pal8, const uint8_t* scratch, uint8_t* frame, uint32_t* total_host, int w, int h, hipStream_t s, hipEvent_t done) {
    gif_pack(pal8 + (size_t)w * h, scratch, frame, total_host, gif_segments(w, h), s, done);
}

void launch_gif_lzw_bgr(const uint8_t* bgr, const uint8_t* seq_tables, uint8_t* scratch, int w, int h, hipStream_t s) {
    const int n_seg = gif_segments(w, h);
    hipLaunchKernelGGL(k_gif_lzw_bgr, dim3((unsigned)((n_seg + kLzwWaves - 1) / kLzwWaves)), dim3(64 * kLzwWaves), 0, s, bgr, seq_tables + kPal8SeqTableOffset, (uint32_t*)scratch,
                       gif_lengths(scratch, n_seg), (int)((size_t)w * h), n_seg);
}

void launch_gif_pack_seq(const uint8_t* seq_tables, const uint8_t* scratch, uint8_t* frame, uint32_t* total_host, int w, int h, hipStream_t s, hipEvent_t done) {
    gif_pack(seq_tables + kPal8SeqPaletteOffset, scratch, frame, total_host, gif_segments(w, h), s, done);
}

size_t gif_scratch_bytes(int w, int h) {
    const size_t n_seg = ((size_t)w * h + kSeg - 1) / kSeg;
    return n_seg * (kGifSlotBytes + 4) + 16;
}

}  // namespace poppy_hip
