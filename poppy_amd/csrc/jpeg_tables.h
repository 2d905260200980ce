// jpeg_tables.h — the constants of the POPPY_FRAME_JPEG hand-off format (include/poppy_hip.h has the rule) that the host statement (frame_jpeg.cpp) and the device
// coder (kernels_frame_jpeg.hip) share: the Annex K quantisation and Huffman tables of ITU-T T.81, the zig-zag order, the DCT's integer cosines, the fixed
// header's layout, the quality scaling, and the block of per-quality tables the kernels read.  Host and device, nothing of HIP.
#pragma once
#include "../../include/poppy_hip.h"
#include <cstddef>
#include <cstdint>

namespace poppy_hip {
namespace jpeg {

// zig-zag position -> natural index (row * 8 + column)
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 Annex K.1, tables K.1 (luminance) and K.2 (chrominance), natural order
constexpr uint8_t kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// T.81 Annex K.3, the "typical" Huffman tables: the number of codes of each length 1..16, then the symbols in code order
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};      // (both DC tables)
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// The DCT's integer cosines: kCos[k] = round(8192 * cos(k * pi / 16)).  T[u][x] = round(2^14 * a(u) * cos((2 x + 1) u pi / 16)) with a(0) = sqrt(1 / 8),
// a(u) = 1 / 2 is +-kCos[(2 x + 1) u reduced to 0..7] for u > 0 and kCos[4] = 5793 for u = 0 (dct_entry).
constexpr int kCos[8] = {8192, 8035, 7568, 6811, 5793, 4551, 3135, 1598};
constexpr int dct_entry(int u, int x) {
    if (u == 0) return kCos[4];
    int k = ((2 * x + 1) * u) % 32;                         // cos(k pi / 16), period 32, even around 0 and 16, odd around 8
    if (k > 16) k = 32 - k;
    return k <= 8 ? (k == 8 ? 0 : kCos[k]) : -kCos[16 - k];
}
constexpr int kDctPass1Shift = 11, kDctPass2Shift = 14;     // after them a coefficient is 8 times the orthonormal DCT's (3 fractional bits)

// quality -> a table's entry (libjpeg's jpeg_quality_scaling and jpeg_add_quant_table with force_baseline)
constexpr int quant_entry(int table, int natural, int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = (kBaseQuant[table][natural] * scale + 50) / 100;
    return v < 1 ? 1 : v > 255 ? 255 : v;
}

// the fixed header (include/poppy_hip.h lists its segments): offsets inside the JFIF file, which begins at the frame's byte 4
constexpr int kHeaderBytes = 613;
constexpr int kOffDqt = 20 + 4, kOffSofHeight = 154 + 5, kOffDht = 173, kOffDri = 593, kOffSos = 599;      // kOffDqt: the first table's Pq/Tq byte; the second's is 65 further
constexpr size_t kFrameData = 4 + kHeaderBytes;             // the frame's offset of the entropy-coded data

// One Huffman table as the coders look it up: entry = code << 8 | length (0: no such symbol).  DC tables have 12 symbols, AC tables 256.
struct HuffTables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
constexpr void huff_fill(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
    uint32_t code = 0;
    int at = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[at++]] = code++ << 8 | (uint32_t)len;
        code <<= 1;
    }
}
constexpr HuffTables make_huff() {
    HuffTables h{};
    for (int t = 0; t < 2; ++t) { huff_fill(kDcBits[t], kDcVals, h.dc[t]); huff_fill(kAcBits[t], kAcVals[t], h.ac[t]); }
    return h;
}

// What the kernels read per quality: the header's bytes with the two tables in it (width and height are the pack kernel's to fill in), and per table and natural
// index the quantiser's rounding bias 4 Q and the reciprocal of its divisor 8 Q, m = ceil(2^32 / (8 Q)): (n * m) >> 32 == n / (8 Q) for every n < 2^15
// (m * 8 Q - 2^32 < 8 Q <= 2040 < 2^11, so the product's error stays below 2^32 * 2^-6; tests/test_host_jpeg.py checks the identity for every n and Q).
struct QualityTables {
    uint8_t header[kHeaderBytes + 3];
    uint32_t bias[2][64];
    uint32_t recip[2][64];
};
constexpr uint32_t quant_recip(int q) { return (uint32_t)(((1ull << 32) + 8ull * q - 1) / (8ull * q)); }
void fill_quality_tables(int quality, QualityTables* t);      // frame_jpeg.cpp
void write_header(int quality, int width, int height, uint8_t* dst);      // kHeaderBytes bytes (POPPY_FRAME_JPEG's: 4:2:0)
// the host coder with an interval of its caller's choice (the format's is kRestartMcus; another one is for measuring what the choice costs); returns `total`
size_t encode_i420(const uint8_t* i420, int w, int h, int quality, int restart_mcus, uint8_t* dst);

constexpr int kRestartMcus = POPPY_JPEG_RESTART_MCUS;

// The sampling of a JPEG hand-off format: POPPY_FRAME_JPEG codes the I420 planes (an MCU is 16 x 16 samples, six blocks), POPPY_FRAME_JPEG444 the I444 planes
// (8 x 8 samples, three blocks).  Everything else of the two rules is one rule; these are the facts that differ.
enum Sampling { k420 = 0, k444 = 1 };
constexpr int kRestartMcus444 = POPPY_JPEG444_RESTART_MCUS;
constexpr int mcu_blocks(Sampling s) { return s == k444 ? 3 : 6; }
constexpr int mcu_side(Sampling s) { return s == k444 ? 8 : 16; }      // an MCU's side in samples of the frame
constexpr int restart_mcus(Sampling s) { return s == k444 ? kRestartMcus444 : kRestartMcus; }
// the two header bytes in which the formats differ: SOF0 component 1's sampling factors, DRI's low byte (the interval)
constexpr int kOffSofSampling = 154 + 11, kOffDriLow = 593 + 5;
constexpr uint8_t sof_sampling(Sampling s) { return s == k444 ? 0x11 : 0x22; }
static_assert(mcu_blocks(k444) * kRestartMcus444 == mcu_blocks(k420) * kRestartMcus,
              "a 4:4:4 segment has the blocks of a 4:2:0 segment: POPPY_JPEG_SEGMENT_BYTES bounds it, and the coder's lanes, bit buffer and scratch slot serve both");
// the host coder of either sampling on its planes (I420 or I444) with the format's interval; returns `total`
size_t encode_planes(const uint8_t* planes, int w, int h, int quality, Sampling s, uint8_t* dst);
// the bound of a coded block in bits, of a segment in bytes behind stuffing with its marker, and of a frame (include/poppy_hip.h: Capacity)
constexpr size_t kBlockBitsMax = 11 + 11 + 63 * (16 + 10);
constexpr size_t kSegmentBytesMax = POPPY_JPEG_SEGMENT_BYTES;
static_assert(kSegmentBytesMax == 2 * ((6 * kBlockBitsMax * kRestartMcus + 7) / 8) + 2, "POPPY_JPEG_SEGMENT_BYTES is the header's bound");
inline size_t mcu_count(size_t w, size_t h, Sampling s = k420) { const size_t m = (size_t)mcu_side(s); return ((w + m - 1) / m) * ((h + m - 1) / m); }
inline size_t segment_count(size_t w, size_t h, Sampling s = k420) { return (mcu_count(w, h, s) + restart_mcus(s) - 1) / restart_mcus(s); }
inline unsigned long long frame_capacity(size_t w, size_t h, Sampling s = k420) { return kFrameData + (unsigned long long)segment_count(w, h, s) * kSegmentBytesMax; }
constexpr size_t kFrameMinBytes = kFrameData + 1 + 2;       // the smallest frame: a byte of entropy data and EOI

// ---- POPPY_FRAME_JPEG_OPT and POPPY_FRAME_JPEG444_OPT: the same files on four Huffman tables built from the frame's own symbol counts (include/poppy_hip.h) ----
// A frame's symbol counts, laid out as the lookup tables are: dc[t][category], ac[t][run << 4 | size].  The DHT's table k = 0..3 is DC 0, AC 0, DC 1, AC 1:
// class k & 1, id k >> 1.
using SymbolCounts = HuffTables;
constexpr int kCountWords = (int)(sizeof(SymbolCounts) / 4);
constexpr uint32_t* table_of(HuffTables& h, int k) { return k & 1 ? h.ac[k >> 1] : h.dc[k >> 1]; }
constexpr int table_symbols(int k) { return k & 1 ? 256 : 16; }
// the header: POPPY_FRAME_JPEG's up to the DHT marker, the DHT's marker and length, per table 17 bytes and its values, DRI and SOS as they were
constexpr int kOptHeaderFixed = kOffDht + 4 + (kHeaderBytes - kOffDri);
constexpr int kOptHeaderMax = kOptHeaderFixed + 2 * (17 + 12) + 2 * (17 + 162);      // a DC table has at most 12 symbols, an AC table 16 x 10 run / size pairs, EOB and ZRL
static_assert(kOptHeaderFixed == 197 && kOptHeaderMax == kHeaderBytes, "the OPT header is 197 + sum(17 + n) bytes, at most the fixed header's 613");
// What the device's table build leaves for the coder and the gather: the lookup entries, and per DHT table its n and its bytes (class / id, bits, n values)
struct OptTables {
    HuffTables huff;
    uint32_t n[4];
    uint8_t dht[4][17 + 256 + 3];
};
// a code may have 16 bits whatever the table, and a DC tree has at most 13 leaves (12 categories and the reserved entry): a DC code has at most 12 bits
constexpr size_t kOptBlockBitsMax = 12 + 11 + 63 * (16 + 10);
constexpr size_t kOptSegmentBytesMax = POPPY_JPEG_OPT_SEGMENT_BYTES;
static_assert(kOptSegmentBytesMax == 2 * ((6 * kOptBlockBitsMax * kRestartMcus + 7) / 8) + 2, "POPPY_JPEG_OPT_SEGMENT_BYTES is the header's bound");
inline unsigned long long opt_frame_capacity(size_t w, size_t h, Sampling s = k420) { return 4 + kOptHeaderMax + (unsigned long long)segment_count(w, h, s) * kOptSegmentBytesMax; }
constexpr size_t kOptFrameMinBytes = 4 + kOptHeaderFixed + 4 * (17 + 1) + 1 + 2;      // four one-symbol tables, a byte of entropy data, EOI
// the host coder of either sampling on per-frame tables; returns `total`
size_t encode_planes_opt(const uint8_t* planes, int w, int h, int quality, Sampling s, uint8_t* dst);
// ... and on one table set per sequence (POPPY_FRAME_JPEG_SEQ, POPPY_FRAME_JPEG444_SEQ): n frames of planes frame_stride bytes apart, every frame standing for
// `copies` of itself in the sums (the phase 0 / 1 copies; otherwise 1); frame k goes to dst + k * dst_stride
void encode_planes_seq(const uint8_t* planes, size_t frame_stride, int n, int copies, int w, int h, int quality, Sampling s, uint8_t* dst, size_t dst_stride);

// ---- the byte budgets (include/poppy_hip.h, "JPEG byte budget" and "JPEG sequence budget"): the rule, written once.  size(q): the length in bytes of what the
// budget is about at quality q — a frame's file, or the sum of a sequence's files —, asked about at most 1 + ceil(log2(quality_max)) times. ----
template <class Size>
int budget_search(Size size, int quality_max, unsigned long long budget) {
    if (size(quality_max) <= budget) return quality_max;
    int lo = 0, hi = quality_max;                           // hi is known not to fit; lo = 0: nothing known to fit
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (size(mid) <= budget) lo = mid; else hi = mid;
    }
    return lo > 1 ? lo : 1;
}

}  // namespace jpeg
}  // namespace poppy_hip
