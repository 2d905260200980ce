// kernels_frame_pal8.hip — the frame a slot rendered (tight u8x3 BGR) -> PAL8 for the writer hand-off (include/poppy_hip.h: POPPY_FRAME_PAL8):
// one index byte per pixel + a 768-byte R, G, B palette built per frame by a median cut over the 32^3 cells (R >> 3, G >> 3, B >> 3).
// poppy_bgr_to_pal8 (frame_pal8.cpp) is the host statement of the same integer arithmetic; the bytes are equal.
//
// Three dispatches, no host round trip (phase-mode bodies are captured graphs, chained frames are queued ahead):
//   k_pal8_hist   the frame read once as a linear run of pixels (the frame is tight, so rows do not matter), four pixels per thread.  Per cell
//                 two 64-bit words: A = count << 32 | sum R, B = sum B << 32 | sum G (a frame has at most 2^24 pixels, so no field carries
//                 into its neighbour).  A thread first merges the equal cells among its four neighbouring pixels, then adds into a 2048-entry
//                 hash table of its workgroup in LDS (morph frames are smooth: a workgroup's pixels fall into a few hundred cells); a cell
//                 that finds no place within eight probes goes to the global tables directly.  The workgroup's table is added to the global
//                 tables at the end: two 64-bit vector atomics per occupied entry instead of two per pixel.
//   k_pal8_build  ONE workgroup.  The counts' 3-D inclusive prefix sums in LDS (33^3 words, 140 KiB; three axis scans by all 1024 threads), then the at most
//                 255 cuts by wave 0 alone: with the prefix sums a box's count, its marginal along an axis and its bounding box are eight
//                 look-ups per lane, lanes over cut positions; the boxes live in the wave's registers, four per lane, and the arg-max is a
//                 wave reduction of the score and a ballot for its lowest index.  Then all 16 waves, a box each: the cell -> index table, the box's colour
//                 sums and its palette entry.  The cells read are cleared on the way, so the tables are zero again for the slot's next frame.
//   k_pal8_remap  index = table[cell], four pixels per thread, one 4-byte store.
//
// POPPY_FRAME_PAL8_SEQ (one palette for all frames of a sequence; poppy_bgr_frames_to_pal8 is its host statement) uses the same pieces around tables that live for a
// whole sequence:
//   k_pal8_seq_pass   per frame: k_pal8_hist's read and LDS stage (the packed words are safe inside one workgroup), but every occupied entry is flushed UNPACKED into
//                     four 64-bit tables (count, sum R, sum G, sum B: packed fields would carry into each other when summed over frames), and the pixels just read
//                     are stored on into the frame's place in the sequence store — the pass is the frame's only conversion work before the last frame.
//   k_pal8_seq_build  once per sequence: k_pal8_build's code (pal8_build<true>) on those tables; counts go into the 32-bit prefix array (a sequence has fewer
//                     than 2^32 pixels), scores (count * side, up to 2^37) and colour sums are 64-bit.
//   k_pal8_remap      per frame, from the store.
#include "kernels.h"
#include "pal8_cells.h"
#include <hip/hip_ext.h>
#include <algorithm>
#include <mutex>
#include <type_traits>

namespace poppy_hip {

namespace {

constexpr int kCells = 32768;
constexpr int kHistSlots = 2048;                 // per workgroup: 8 KiB of keys + 2 x 16 KiB of sums
constexpr int kHistProbes = 8;

}  // namespace

__global__ void __launch_bounds__(256) k_pal8_hist(const uint8_t* __restrict__ src, unsigned long long* __restrict__ hist_a, unsigned long long* __restrict__ hist_b,
                                                   size_t n_px, int aligned) {
    __shared__ int keys[kHistSlots];
    __shared__ unsigned long long va[kHistSlots], vb[kHistSlots];
    for (int i = threadIdx.x; i < kHistSlots; i += 256) { keys[i] = -1; va[i] = 0; vb[i] = 0; }
    __syncthreads();
    auto add = [&](int cell, unsigned long long a, unsigned long long b) {
        unsigned h = ((unsigned)cell * 2654435761u) >> 21;           // 11 bits
        for (int p = 0; p < kHistProbes; ++p) {
            const int prev = atomicCAS(&keys[h], -1, cell);
            if (prev == -1 || prev == cell) { atomicAdd(&va[h], a); atomicAdd(&vb[h], b); return; }
            h = (h + 1) & (kHistSlots - 1);
        }
        atomicAdd(&hist_a[cell], a); atomicAdd(&hist_b[cell], b);
    };
    const size_t n_quads = (n_px + 3) / 4;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n_quads; q += (size_t)gridDim.x * 256) {
        const int n = n_px - q * 4 >= 4 ? 4 : (int)(n_px - q * 4);
        uint32_t w[3];
        load_quad(src, q, n, aligned != 0, w);
        int cur = -1;
        unsigned long long a = 0, b = 0;
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < n) {
                const int pb = quad_byte(w, 3 * k), pg = quad_byte(w, 3 * k + 1), pr = quad_byte(w, 3 * k + 2);
                const int cell = cell_of(pb, pg, pr);
                if (cell != cur) { if (cur >= 0) add(cur, a, b); cur = cell; a = 0; b = 0; }
                a += (1ull << 32) | (unsigned long long)pr;
                b += ((unsigned long long)pb << 32) | (unsigned long long)pg;
            }
        }
        if (cur >= 0) add(cur, a, b);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kHistSlots; i += 256) {
        const int cell = keys[i];
        if (cell >= 0) { atomicAdd(&hist_a[cell], va[i]); atomicAdd(&hist_b[cell], vb[i]); }
    }
}

// tab: four tables of kCells 64-bit words (count, sum R, sum G, sum B).  store (may be null): where the frame's bytes go, as they are.
__global__ void __launch_bounds__(256) k_pal8_seq_pass(const uint8_t* __restrict__ src, uint8_t* __restrict__ store, unsigned long long* __restrict__ tab, size_t n_px, int aligned) {
    __shared__ int keys[kHistSlots];
    __shared__ unsigned long long va[kHistSlots], vb[kHistSlots];
    for (int i = threadIdx.x; i < kHistSlots; i += 256) { keys[i] = -1; va[i] = 0; vb[i] = 0; }
    __syncthreads();
    auto flush = [&](int cell, unsigned long long a, unsigned long long b) {
        atomicAdd(&tab[cell], a >> 32); atomicAdd(&tab[kCells + cell], a & 0xffffffffull);
        atomicAdd(&tab[2 * kCells + cell], b & 0xffffffffull); atomicAdd(&tab[3 * kCells + cell], b >> 32);
    };
    auto add = [&](int cell, unsigned long long a, unsigned long long b) {
        unsigned h = ((unsigned)cell * 2654435761u) >> 21;           // 11 bits
        for (int p = 0; p < kHistProbes; ++p) {
            const int prev = atomicCAS(&keys[h], -1, cell);
            if (prev == -1 || prev == cell) { atomicAdd(&va[h], a); atomicAdd(&vb[h], b); return; }
            h = (h + 1) & (kHistSlots - 1);
        }
        flush(cell, a, b);
    };
    const size_t n_quads = (n_px + 3) / 4;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n_quads; q += (size_t)gridDim.x * 256) {
        const int n = n_px - q * 4 >= 4 ? 4 : (int)(n_px - q * 4);
        uint32_t w[3];
        load_quad(src, q, n, aligned != 0, w);
        if (store) {
            if (aligned && n == 4) { uint32_t* o = (uint32_t*)(store + q * 12); o[0] = w[0]; o[1] = w[1]; o[2] = w[2]; }
            else for (int i = 0; i < 3 * n; ++i) store[q * 12 + i] = (uint8_t)quad_byte(w, i);
        }
        int cur = -1;
        unsigned long long a = 0, b = 0;
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < n) {
                const int pb = quad_byte(w, 3 * k), pg = quad_byte(w, 3 * k + 1), pr = quad_byte(w, 3 * k + 2);
                const int cell = cell_of(pb, pg, pr);
                if (cell != cur) { if (cur >= 0) add(cur, a, b); cur = cell; a = 0; b = 0; }
                a += (1ull << 32) | (unsigned long long)pr;
                b += ((unsigned long long)pb << 32) | (unsigned long long)pg;
            }
        }
        if (cur >= 0) add(cur, a, b);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kHistSlots; i += 256) {
        const int cell = keys[i];
        if (cell >= 0) flush(cell, va[i], vb[i]);
    }
}

namespace {

// The counts' inclusive prefix sums live in a 33^3 array whose planes r = -1, g = -1 and b = -1 are zero, so that a box's count is eight plain look-ups:
// (r, g, b) is at (r + 1) * 1089 + (g + 1) * 33 + (b + 1).
constexpr int kPrefR = 33 * 33, kPrefG = 33, kPrefWords = 33 * 33 * 33;
constexpr unsigned kBuildLds = kPrefWords * 4;

struct Box3 { int r0, g0, b0, r1, g1, b1; };

// pixels in the cells of x (mod 2^32 arithmetic; the result is exact)
__device__ __forceinline__ uint32_t box_count(const uint32_t* P, int r0, int g0, int b0, int r1, int g1, int b1) {
    const int R0 = r0 * kPrefR, R1 = (r1 + 1) * kPrefR, G0 = g0 * kPrefG, G1 = (g1 + 1) * kPrefG, B0 = b0, B1 = b1 + 1;
    return P[R1 + G1 + B1] - P[R0 + G1 + B1] - P[R1 + G0 + B1] - P[R1 + G1 + B0] + P[R0 + G0 + B1] + P[R0 + G1 + B0] + P[R1 + G0 + B0] - P[R0 + G0 + B0];
}

// a box's corners in 30 bits: lo r, g, b, hi r, g, b, five bits each
__device__ __forceinline__ uint32_t pack_box(const Box3& x) {
    return (uint32_t)x.r0 | (uint32_t)x.g0 << 5 | (uint32_t)x.b0 << 10 | (uint32_t)x.r1 << 15 | (uint32_t)x.g1 << 20 | (uint32_t)x.b1 << 25;
}
__device__ __forceinline__ Box3 unpack_box(uint32_t v) {
    Box3 x;
    x.r0 = v & 31; x.g0 = (v >> 5) & 31; x.b0 = (v >> 10) & 31; x.r1 = (v >> 15) & 31; x.g1 = (v >> 20) & 31; x.b1 = (v >> 25) & 31;
    return x;
}
// count * (longest side in cells), 0 for a box of one cell; at most 2^24 * 32 for a frame (Score = uint32_t), below 2^32 * 32 for a sequence (64-bit)
template <typename Score>
__device__ __forceinline__ Score box_score(uint32_t lh, uint32_t count) {
    const Box3 x = unpack_box(lh);
    const int side = max(max(x.r1 - x.r0, x.g1 - x.g0), x.b1 - x.b0) + 1;
    return side < 2 ? (Score)0 : (Score)count * (Score)side;
}

// Wave 0, all 64 lanes.  Two boxes at once, lanes 0..31 on a and 32..63 on b, holding ca > 0 and cb > 0 pixels: both shrunk to the bounding boxes of
// their occupied cells.  Lane p of a half takes position lo + p of every axis: the pixels at coordinates <= that position are none before the first
// occupied slab and all from the last one on.  The results are uniform over the wave.
__device__ __forceinline__ void shrink_pair(const uint32_t* P, Box3& a, Box3& b, uint32_t ca, uint32_t cb) {
    const int lane = threadIdx.x & 63, p = lane & 31;
    const bool up = lane >= 32;
    const int r0 = up ? b.r0 : a.r0, g0 = up ? b.g0 : a.g0, b0 = up ? b.b0 : a.b0, r1 = up ? b.r1 : a.r1, g1 = up ? b.g1 : a.g1, b1 = up ? b.b1 : a.b1;
    const uint32_t tot = up ? cb : ca;
    const uint32_t cum_r = box_count(P, r0, g0, b0, min(r0 + p, r1), g1, b1);
    const uint32_t cum_g = box_count(P, r0, g0, b0, r1, min(g0 + p, g1), b1);
    const uint32_t cum_b = box_count(P, r0, g0, b0, r1, g1, min(b0 + p, b1));
    const bool vr = r0 + p <= r1, vg = g0 + p <= g1, vb = b0 + p <= b1;
    const unsigned long long fr = __ballot(vr && cum_r > 0), lr = __ballot(vr && cum_r == tot);
    const unsigned long long fg = __ballot(vg && cum_g > 0), lg = __ballot(vg && cum_g == tot);
    const unsigned long long fb = __ballot(vb && cum_b > 0), lb = __ballot(vb && cum_b == tot);
    auto first = [](unsigned long long m, int half) { return __ffs((uint32_t)(m >> (32 * half))) - 1; };
    { const int o = a.r0; a.r0 = o + first(fr, 0); a.r1 = o + first(lr, 0); }
    { const int o = a.g0; a.g0 = o + first(fg, 0); a.g1 = o + first(lg, 0); }
    { const int o = a.b0; a.b0 = o + first(fb, 0); a.b1 = o + first(lb, 0); }
    { const int o = b.r0; b.r0 = o + first(fr, 1); b.r1 = o + first(lr, 1); }
    { const int o = b.g0; b.g0 = o + first(fg, 1); b.g1 = o + first(lg, 1); }
    { const int o = b.b0; b.b0 = o + first(fb, 1); b.b1 = o + first(lb, 1); }
}

}  // namespace

// The palette build, for one frame (kSeq = false: hist_a / hist_b are k_pal8_hist's packed words) and for a sequence (kSeq = true: hist_a is k_pal8_seq_pass's four
// unpacked tables, hist_b is not used).  The two differ in where a cell's count and sums are read and in the width of the scores and colour sums, nowhere else.
namespace {
template <bool kSeq>
__device__ __forceinline__ void pal8_build(unsigned long long* __restrict__ hist_a, unsigned long long* __restrict__ hist_b, uint8_t* __restrict__ table,
                                           uint8_t* __restrict__ palette) {
    using Score = typename std::conditional<kSeq, unsigned long long, uint32_t>::type;
    using Sum = Score;
    extern __shared__ uint32_t P[];                       // kPrefWords
    __shared__ uint32_t box_lh[256], box_cnt[256];
    __shared__ int n_boxes_s;
    const int t = threadIdx.x, lane = t & 63;
    for (int i = t; i < kPrefWords; i += 1024) P[i] = 0;
    __syncthreads();
    // along B: 32 consecutive cells are one (r, g) row and one half of a wave
    for (int it = 0; it < 32; ++it) {
        const int cell = it * 1024 + t;
        uint32_t v = kSeq ? (uint32_t)hist_a[cell] : (uint32_t)(hist_a[cell] >> 32);
        #pragma unroll
        for (int d = 1; d < 32; d <<= 1) { const uint32_t u = __shfl_up(v, d, 32); if ((lane & 31) >= d) v += u; }
        P[((cell >> 10) + 1) * kPrefR + (((cell >> 5) & 31) + 1) * kPrefG + (cell & 31) + 1] = v;
    }
    __syncthreads();
    { const int r = t >> 5, b = t & 31; uint32_t acc = 0; for (int g = 0; g < 32; ++g) { const int i = (r + 1) * kPrefR + (g + 1) * kPrefG + b + 1; acc += P[i]; P[i] = acc; } }      // along G
    __syncthreads();
    { const int g = t >> 5, b = t & 31; uint32_t acc = 0; for (int r = 0; r < 32; ++r) { const int i = (r + 1) * kPrefR + (g + 1) * kPrefG + b + 1; acc += P[i]; P[i] = acc; } }      // along R
    __syncthreads();
    if (t < 64) {
        uint32_t lh0 = 0, lh1 = 0, lh2 = 0, lh3 = 0, cn0 = 0, cn1 = 0, cn2 = 0, cn3 = 0;       // boxes lane, lane + 64, lane + 128, lane + 192
        int n = 1;
        {
            Box3 a = {0, 0, 0, 31, 31, 31}, b = a;
            const uint32_t total = P[kPrefWords - 1];
            shrink_pair(P, a, b, total, total);
            if (lane == 0) { lh0 = pack_box(a); cn0 = total; }
        }
        while (n < 256) {
            // the best score at the lowest index (boxes that do not exist score 0)
            const Score s0 = box_score<Score>(lh0, cn0), s1 = box_score<Score>(lh1, cn1), s2 = box_score<Score>(lh2, cn2), s3 = box_score<Score>(lh3, cn3);
            Score m = max(max(s0, s1), max(s2, s3));
            #pragma unroll
            for (int d = 32; d >= 1; d >>= 1) m = max(m, (Score)__shfl_xor(m, d, 64));
            if (m == 0) break;                                      // no box spans more than one cell
            int best;
            unsigned long long w;
            if ((w = __ballot(s0 == m))) best = __ffsll(w) - 1;
            else if ((w = __ballot(s1 == m))) best = 64 + __ffsll(w) - 1;
            else if ((w = __ballot(s2 == m))) best = 128 + __ffsll(w) - 1;
            else { w = __ballot(s3 == m); best = 192 + __ffsll(w) - 1; }
            const int bj = best >> 6;
            const uint32_t my_lh = bj == 0 ? lh0 : bj == 1 ? lh1 : bj == 2 ? lh2 : lh3, my_cnt = bj == 0 ? cn0 : bj == 1 ? cn1 : bj == 2 ? cn2 : cn3;
            const uint32_t blh = __shfl(my_lh, best & 63, 64), bcnt = __shfl(my_cnt, best & 63, 64);
            const Box3 x = unpack_box(blh);
            const int er = x.r1 - x.r0, eg = x.g1 - x.g0, eb = x.b1 - x.b0;
            int axis = 1, ea = eg;                                  // the longest side; ties: G, then R, then B
            if (er > ea) { axis = 0; ea = er; }
            if (eb > ea) { axis = 2; ea = eb; }
            const int la = axis == 0 ? x.r0 : axis == 1 ? x.g0 : x.b0;
            const int pos = la + min(lane, ea);
            const uint32_t cum = box_count(P, x.r0, x.g0, x.b0, axis == 0 ? pos : x.r1, axis == 1 ? pos : x.g1, axis == 2 ? pos : x.b1);
            const uint32_t half = (uint32_t)(((unsigned long long)bcnt + 1) / 2);      // (a sequence's count may be 2^32 - 1)
            const unsigned long long reach = __ballot(lane <= ea && cum >= half);      // never empty: the last position holds them all
            const int k = min(__ffsll(reach) - 1, ea - 1);
            const uint32_t cnt_lo = __shfl(cum, k, 64), cnt_hi = bcnt - cnt_lo;
            Box3 a = x, b = x;
            if (axis == 0) { a.r1 = la + k; b.r0 = la + k + 1; }
            else if (axis == 1) { a.g1 = la + k; b.g0 = la + k + 1; }
            else { a.b1 = la + k; b.b0 = la + k + 1; }
            shrink_pair(P, a, b, cnt_lo, cnt_hi);
            const uint32_t new_lo = pack_box(a), new_hi = pack_box(b);
            if (lane == best) { lh0 = new_lo; cn0 = cnt_lo; } else if (lane + 64 == best) { lh1 = new_lo; cn1 = cnt_lo; }
            else if (lane + 128 == best) { lh2 = new_lo; cn2 = cnt_lo; } else if (lane + 192 == best) { lh3 = new_lo; cn3 = cnt_lo; }
            if (lane == n) { lh0 = new_hi; cn0 = cnt_hi; } else if (lane + 64 == n) { lh1 = new_hi; cn1 = cnt_hi; }
            else if (lane + 128 == n) { lh2 = new_hi; cn2 = cnt_hi; } else if (lane + 192 == n) { lh3 = new_hi; cn3 = cnt_hi; }
            ++n;
        }
        box_lh[lane] = lh0; box_lh[64 + lane] = lh1; box_lh[128 + lane] = lh2; box_lh[192 + lane] = lh3;
        box_cnt[lane] = cn0; box_cnt[64 + lane] = cn1; box_cnt[128 + lane] = cn2; box_cnt[192 + lane] = cn3;
        if (lane == 0) n_boxes_s = n;
    }
    __syncthreads();
    const int n = n_boxes_s;
    // a wave per box: the table, the colour sums (the tables' cells go back to zero), the palette entry
    for (int i = t >> 6; i < n; i += 16) {
        const Box3 x = unpack_box(box_lh[i]);
        const int dg = x.g1 - x.g0 + 1, db = x.b1 - x.b0 + 1, vol = (x.r1 - x.r0 + 1) * dg * db;
        Sum s0 = 0, s1 = 0, s2 = 0;
        for (int v = lane; v < vol; v += 64) {
            const int b = v % db, g = (v / db) % dg, r = v / (db * dg);
            const int cell = ((x.r0 + r) << 10) | ((x.g0 + g) << 5) | (x.b0 + b);
            table[cell] = (uint8_t)i;
            const unsigned long long a = hist_a[cell];
            if (a) {
                if (kSeq) {
                    s0 += (Sum)hist_a[kCells + cell]; s1 += (Sum)hist_a[2 * kCells + cell]; s2 += (Sum)hist_a[3 * kCells + cell];
                    hist_a[cell] = 0; hist_a[kCells + cell] = 0; hist_a[2 * kCells + cell] = 0; hist_a[3 * kCells + cell] = 0;
                } else {
                    const unsigned long long gb = hist_b[cell];
                    s0 += (uint32_t)a; s1 += (uint32_t)gb; s2 += (uint32_t)(gb >> 32);
                    hist_a[cell] = 0; hist_b[cell] = 0;
                }
            }
        }
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { s0 += __shfl_xor(s0, d, 64); s1 += __shfl_xor(s1, d, 64); s2 += __shfl_xor(s2, d, 64); }
        if (lane == 0) {
            const unsigned long long count = box_cnt[i];
            palette[3 * i] = (uint8_t)(((unsigned long long)s0 + count / 2) / count);
            palette[3 * i + 1] = (uint8_t)(((unsigned long long)s1 + count / 2) / count);
            palette[3 * i + 2] = (uint8_t)(((unsigned long long)s2 + count / 2) / count);
        }
    }
    for (int i = n * 3 + t; i < 768; i += 1024) palette[i] = 0;
}
}  // namespace

__global__ void __launch_bounds__(1024) k_pal8_build(unsigned long long* __restrict__ hist_a, unsigned long long* __restrict__ hist_b, uint8_t* __restrict__ table,
                                                     uint8_t* __restrict__ palette) {
    pal8_build<false>(hist_a, hist_b, table, palette);
}

__global__ void __launch_bounds__(1024) k_pal8_seq_build(unsigned long long* __restrict__ tab, uint8_t* __restrict__ table, uint8_t* __restrict__ palette) {
    pal8_build<true>(tab, nullptr, table, palette);
}

__global__ void __launch_bounds__(256) k_pal8_remap(const uint8_t* __restrict__ src, const uint8_t* __restrict__ table, uint8_t* __restrict__ dst, size_t n_px, int aligned) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q * 4 >= n_px) return;
    const int n = n_px - q * 4 >= 4 ? 4 : (int)(n_px - q * 4);
    uint32_t w[3];
    load_quad(src, q, n, aligned != 0, w);
    uint32_t out = 0;
    #pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n) out |= (uint32_t)table[cell_of(quad_byte(w, 3 * k), quad_byte(w, 3 * k + 1), quad_byte(w, 3 * k + 2))] << (8 * k);
    if (aligned && n == 4) *(uint32_t*)(dst + q * 4) = out;
    else for (int k = 0; k < n; ++k) dst[q * 4 + k] = (uint8_t)(out >> (8 * k));
}

// The dynamic-LDS limit of a kernel is process state per device (kernels_pyramid_tail.hip: prepare_pyr_tail): raised once on each device a context
// converts on, with that device current, outside any stream capture.
bool prepare_pal8() {
    static std::mutex mu;
    static bool granted[64] = {false};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    std::lock_guard<std::mutex> lock(mu);
    if (granted[dev]) return true;
    if (hipFuncSetAttribute((const void*)k_pal8_build, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBuildLds) != hipSuccess) return false;
    if (hipFuncSetAttribute((const void*)k_pal8_seq_build, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBuildLds) != hipSuccess) return false;
    granted[dev] = true;
    return true;
}

void launch_pal8_hist(const uint8_t* src, uint8_t* tables, int w, int h, hipStream_t s) {
    const size_t n_px = (size_t)w * h, n_quads = (n_px + 3) / 4;
    unsigned long long* hist_a = (unsigned long long*)tables;
    const int blocks = (int)std::min<size_t>((n_quads + 255) / 256, 512);
    hipLaunchKernelGGL(k_pal8_hist, dim3(blocks), dim3(256), 0, s, src, hist_a, hist_a + kCells, n_px, (int)(((uintptr_t)src & 3) == 0));
}

void launch_pal8_build(uint8_t* tables, uint8_t* dst, int w, int h, hipStream_t s) {
    unsigned long long* hist_a = (unsigned long long*)tables;
    hipLaunchKernelGGL(k_pal8_build, dim3(1), dim3(1024), kBuildLds, s, hist_a, hist_a + kCells, tables + kPal8TableOffset, dst + (size_t)w * h);
}

void launch_pal8_remap(const uint8_t* src, const uint8_t* tables, uint8_t* dst, int w, int h, hipStream_t s, hipEvent_t done) {
    const size_t n_px = (size_t)w * h, n_quads = (n_px + 3) / 4;
    const int aligned = (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
    hipExtLaunchKernelGGL(k_pal8_remap, dim3((unsigned)((n_quads + 255) / 256)), dim3(256), 0, s, nullptr, done, 0, src, tables + kPal8TableOffset, dst, n_px, aligned);
}

void launch_pal8_seq_pass(const uint8_t* src, uint8_t* store, uint8_t* seq_tables, int w, int h, hipStream_t s, hipEvent_t done) {
    const size_t n_px = (size_t)w * h, n_quads = (n_px + 3) / 4;
    const int blocks = (int)std::min<size_t>((n_quads + 255) / 256, 512);
    const int aligned = (((uintptr_t)src | (uintptr_t)store) & 3) == 0;
    hipExtLaunchKernelGGL(k_pal8_seq_pass, dim3(blocks), dim3(256), 0, s, nullptr, done, 0, src, store, (unsigned long long*)seq_tables, n_px, aligned);
}

void launch_pal8_seq_build(uint8_t* seq_tables, hipStream_t s) {
    hipLaunchKernelGGL(k_pal8_seq_build, dim3(1), dim3(1024), kBuildLds, s, (unsigned long long*)seq_tables, seq_tables + kPal8SeqTableOffset, seq_tables + kPal8SeqPaletteOffset);
}

void launch_pal8_seq_remap(const uint8_t* src, const uint8_t* seq_tables, uint8_t* dst, int w, int h, hipStream_t s) {
    const size_t n_px = (size_t)w * h, n_quads = (n_px + 3) / 4;
    const int aligned = (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
    hipLaunchKernelGGL(k_pal8_remap, dim3((unsigned)((n_quads + 255) / 256)), dim3(256), 0, s, src, seq_tables + kPal8SeqTableOffset, dst, n_px, aligned);
}

}  // namespace poppy_hip
