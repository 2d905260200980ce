// frame_jpeg.cpp — the library's definition of the POPPY_FRAME_JPEG and POPPY_FRAME_JPEG444 hand-off formats in plain C++ (include/poppy_hip.h has the rule): an
// I420 (an I444) frame coded as one baseline JFIF file in independent restart intervals of POPPY_JPEG_RESTART_MCUS (POPPY_JPEG444_RESTART_MCUS) MCUs.  One coder,
// the sampling its parameter (jpeg_tables.h: Sampling).  kernels_frame_jpeg.hip computes the same bytes on the device, tests/test_host_jpeg.py and
// tests/test_host_jpeg444.py pin these to numpy restatements of the rule.  Host only, integer arithmetic only.
#include "frame_limits.h"
#include <cstring>
#include <vector>

namespace poppy_hip {
namespace jpeg {

namespace {

constexpr HuffTables kHuff = make_huff();

void put16(uint8_t* p, int v) { p[0] = (uint8_t)(v >> 8); p[1] = (uint8_t)v; }

// the header with the tables of `quality`, 4:2:0's; width and height 0 (write_header and the pack kernel fill them in, and the two bytes of the sampling)
void header_template(int quality, uint8_t* h) {
    static const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    memcpy(h, app0, 20);
    uint8_t* p = h + 20;
    p[0] = 0xFF; p[1] = 0xDB; put16(p + 2, 2 + 65 + 65);
    for (int t = 0; t < 2; ++t) {
        p[4 + 65 * t] = (uint8_t)t;                         // Pq = 0 (8-bit entries), Tq = t
        for (int k = 0; k < 64; ++k) p[5 + 65 * t + k] = (uint8_t)quant_entry(t, kZigzag[k], quality);
    }
    p = h + kOffSofHeight - 5;
    static const uint8_t sof[19] = {0xFF, 0xC0, 0, 17, 8, 0, 0, 0, 0, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};
    memcpy(p, sof, 19);
    p = h + kOffDht;
    p[0] = 0xFF; p[1] = 0xC4; put16(p + 2, 2 + 2 * (17 + 12) + 2 * (17 + 162));
    p += 4;
    for (int t = 0; t < 2; ++t) {                           // DC 0, AC 0, DC 1, AC 1
        *p++ = (uint8_t)t; memcpy(p, kDcBits[t], 16); memcpy(p + 16, kDcVals, 12); p += 28;
        *p++ = (uint8_t)(0x10 | t); memcpy(p, kAcBits[t], 16); memcpy(p + 16, kAcVals[t], 162); p += 178;
    }
    static_assert(kOffDht + 4 + 2 * (29 + 179) == kOffDri && kOffDri + 6 == kOffSos && kOffSos + 14 == kHeaderBytes, "the header's layout");
    p[0] = 0xFF; p[1] = 0xDD; put16(p + 2, 4); put16(p + 4, kRestartMcus);
    static const uint8_t sos[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    memcpy(h + kOffSos, sos, 14);
}

// a segment's bits, most significant first
struct BitString {
    std::vector<uint8_t> bytes;
    uint32_t acc = 0; int n_acc = 0;
    void put(uint32_t value, int n) {                       // n <= 16
        acc = acc << n | value; n_acc += n;
        while (n_acc >= 8) { bytes.push_back((uint8_t)(acc >> (n_acc - 8))); n_acc -= 8; }
    }
    void pad() { if (n_acc) put((1u << (8 - n_acc)) - 1, 8 - n_acc); }
};

// sample (x, y) of a w x h plane, the coordinates clamped per axis, level-shifted
inline int sample(const uint8_t* plane, int w, int h, int x, int y) {
    return (int)plane[(size_t)(y < h ? y : h - 1) * w + (x < w ? x : w - 1)] - 128;
}

// the block whose top left sample is (x0, y0): FDCT in two passes and quantisation, the result in zig-zag order
void code_block_coefficients(const uint8_t* plane, int w, int h, int x0, int y0, const QualityTables& q, int table, int16_t* zz) {
    int t[64], f[64];
    for (int y = 0; y < 8; ++y)
        for (int u = 0; u < 8; ++u) {
            int sum = 0;
            for (int x = 0; x < 8; ++x) sum += dct_entry(u, x) * sample(plane, w, h, x0 + x, y0 + y);
            t[y * 8 + u] = (sum + (1 << (kDctPass1Shift - 1))) >> kDctPass1Shift;
        }
    for (int v = 0; v < 8; ++v)
        for (int u = 0; u < 8; ++u) {
            int sum = 0;
            for (int y = 0; y < 8; ++y) sum += dct_entry(v, y) * t[y * 8 + u];
            f[v * 8 + u] = (sum + (1 << (kDctPass2Shift - 1))) >> kDctPass2Shift;
        }
    for (int k = 0; k < 64; ++k) {
        const int n = kZigzag[k], a = f[n] < 0 ? -f[n] : f[n];
        const int m = (int)((a + q.bias[table][n]) / (q.bias[table][n] * 2));      // (|F| + 4 Q) / (8 Q)
        zz[k] = (int16_t)(f[n] < 0 ? -m : m);
    }
}

inline int category(int v) { int a = v < 0 ? -v : v, c = 0; while (a) { ++c; a >>= 1; } return c; }

// One block as its symbols, the one walk of both passes: sink.dc(table, category, difference), then per AC symbol sink.ac(table, symbol, value, category)
// (ZRL and EOB: value 0, category 0).
template <class Sink>
void code_block(Sink& sink, const int16_t* zz, int* pred, int table) {
    const int diff = zz[0] - *pred;
    *pred = zz[0];
    sink.dc(table, category(diff), diff);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        if (zz[k] == 0) { ++run; continue; }
        for (; run >= 16; run -= 16) sink.ac(table, 0xF0, 0, 0);
        const int cat = category(zz[k]);
        sink.ac(table, run << 4 | cat, zz[k], cat);
        run = 0;
    }
    if (run) sink.ac(table, 0, 0, 0);
}

// the coding pass: a symbol's code from the tables it is given, then the value's low bits
struct BitSink {
    BitString& b;
    const HuffTables& huff;
    void put_value(uint32_t code, int v, int cat) {
        b.put(code >> 8, (int)(code & 255));
        if (cat) b.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1), cat);
    }
    void dc(int table, int cat, int diff) { put_value(huff.dc[table][cat], diff, cat); }
    void ac(int table, int symbol, int v, int cat) { put_value(huff.ac[table][symbol], v, cat); }
};
// the counting pass of the per-frame tables
struct CountSink {
    SymbolCounts& n;
    void dc(int table, int cat, int) { ++n.dc[table][cat]; }
    void ac(int table, int symbol, int, int) { ++n.ac[table][symbol]; }
};

}  // namespace

void fill_quality_tables(int quality, QualityTables* t) {
    memset(t, 0, sizeof *t);
    header_template(quality, t->header);
    for (int k = 0; k < 2; ++k)
        for (int n = 0; n < 64; ++n) {
            const int q = quant_entry(k, n, quality);
            t->bias[k][n] = 4u * (uint32_t)q;
            t->recip[k][n] = quant_recip(q);
        }
}

void write_header(int quality, int width, int height, uint8_t* dst) {
    header_template(quality, dst);
    put16(dst + kOffSofHeight, height);
    put16(dst + kOffSofHeight + 2, width);
}

namespace {

// The planes of a frame as their blocks in coding order.  Nothing of the frame is kept: a pass computes each block's coefficients as it reaches it, so the
// two passes of the per-frame tables compute them twice and the frame costs no memory beyond its planes and its bytes.
struct FrameBlocks {
    const uint8_t *yp, *up, *vp;
    int w, h, cw, ch, side, mw, n_mcu;
    Sampling s;
    QualityTables q;
    FrameBlocks(const uint8_t* planes, int w_, int h_, int quality, Sampling s_) : w(w_), h(h_), s(s_) {
        side = mcu_side(s); mw = (w + side - 1) / side; n_mcu = mw * ((h + side - 1) / side);
        cw = s == k444 ? w : (w + 1) / 2; ch = s == k444 ? h : (h + 1) / 2;      // the chroma planes
        yp = planes; up = yp + (size_t)w * h; vp = up + (size_t)cw * ch;
        fill_quality_tables(quality, &q);
    }
    // block k of MCU m: the luma blocks first (2 x 2 of them in a 16 x 16 MCU, one in an 8 x 8 MCU), then Cb, then Cr
    void block(int m, int k, int16_t* zz) const {
        const int mx = m % mw, my = m / mw, luma = mcu_blocks(s) - 2;
        if (k < luma) code_block_coefficients(yp, w, h, side * mx + 8 * (k & 1), side * my + 8 * (k >> 1), q, 0, zz);
        else code_block_coefficients(k == luma ? up : vp, cw, ch, 8 * mx, 8 * my, q, 1, zz);
    }
};

// segment by segment, every block of the frame through `sink`; begin(segment) in front of a segment's first block, end(segment, last) behind its last
template <class Sink, class Begin, class End>
void walk_segments(const FrameBlocks& f, int restart, Sink& sink, Begin begin, End end) {
    const int blocks = mcu_blocks(f.s), luma = blocks - 2;
    int16_t zz[64];
    for (int first = 0, seg = 0; first < f.n_mcu; first += restart, ++seg) {
        begin(seg);
        int pred[3] = {0, 0, 0};
        for (int m = first; m < f.n_mcu && m < first + restart; ++m)
            for (int k = 0; k < blocks; ++k) {
                f.block(m, k, zz);
                code_block(sink, zz, &pred[k < luma ? 0 : k - luma + 1], k >= luma);
            }
        end(seg, first + restart >= f.n_mcu);
    }
}

// the OPT header at dst: the fixed header's bytes around one DHT with the four tables given; returns its length
size_t write_opt_header(int quality, int w, int h, Sampling s, int restart, const uint8_t (*bits)[16], const uint8_t (*vals)[256], const int* n, uint8_t* dst) {
    uint8_t fixed[kHeaderBytes];
    write_header(quality, w, h, fixed);
    fixed[kOffSofSampling] = sof_sampling(s);
    put16(fixed + kOffDri + 4, restart);
    memcpy(dst, fixed, kOffDht);
    uint8_t* p = dst + kOffDht;
    p[0] = 0xFF; p[1] = 0xC4; put16(p + 2, 2 + 4 * 17 + n[0] + n[1] + n[2] + n[3]);
    p += 4;
    for (int k = 0; k < 4; ++k) {                           // DC 0, AC 0, DC 1, AC 1
        *p++ = (uint8_t)((k & 1) << 4 | k >> 1);
        memcpy(p, bits[k], 16); memcpy(p + 16, vals[k], (size_t)n[k]); p += 16 + n[k];
    }
    memcpy(p, fixed + kOffDri, kHeaderBytes - kOffDri);
    return (size_t)(p - dst) + (kHeaderBytes - kOffDri);
}

// the counting pass of one frame: every symbol the coder emits for it, added into `counts`
void count_frame(const FrameBlocks& frame, int restart, SymbolCounts& counts) {
    CountSink counter{counts};
    walk_segments(frame, restart, counter, [](int) {}, [](int, bool) {});
}

// the four tables of the rule on `counts`, as the coder looks them up (`built`), and the OPT header that names them at dst; returns its length
size_t build_opt_tables(SymbolCounts& counts, int quality, int w, int h, Sampling s, int restart, HuffTables* built, uint8_t* dst) {
    uint8_t bits[4][16], vals[4][256];
    int n[4];
    for (int k = 0; k < 4; ++k) {
        uint32_t c[256] = {};
        memcpy(c, table_of(counts, k), sizeof(uint32_t) * table_symbols(k));
        poppy_jpeg_optimal_table(c, bits[k], vals[k], &n[k]);      // (every table of every frame has a symbol, and a frame or sequence the format accepts stays below the sum's limit)
        huff_fill(bits[k], vals[k], table_of(*built, k));
    }
    return write_opt_header(quality, w, h, s, restart, bits, vals, n, dst);
}

// the coding pass of one frame on `huff`: its segments from dst + at on (the header stands in front), then `total` into dst's first four bytes; returns it
size_t code_frame(const FrameBlocks& frame, int restart, const HuffTables& huff, size_t at, uint8_t* dst) {
    BitString b;
    BitSink coder{b, huff};
    walk_segments(frame, restart, coder, [&](int) { b = BitString(); }, [&](int seg, bool last) {
        b.pad();
        for (uint8_t byte : b.bytes) { dst[at++] = byte; if (byte == 0xFF) dst[at++] = 0; }
        dst[at++] = 0xFF;
        dst[at++] = last ? (uint8_t)0xD9 : (uint8_t)(0xD0 + (seg & 7));
    });
    dst[0] = (uint8_t)at; dst[1] = (uint8_t)(at >> 8); dst[2] = (uint8_t)(at >> 16); dst[3] = (uint8_t)(at >> 24);
    return at;
}

// the frame of the planes of sampling `s` with restart intervals of `restart` MCUs (the header's DRI names it), on the Annex K tables or (opt) on the tables
// of the frame's own counts: the counting pass, the table rule, and the same coding pass over the same coefficients on what it gave; returns `total`
size_t encode(const uint8_t* planes, int w, int h, int quality, Sampling s, int restart, bool opt, uint8_t* dst) {
    const FrameBlocks frame(planes, w, h, quality, s);
    if (opt) {
        SymbolCounts counts{};
        HuffTables built{};
        count_frame(frame, restart, counts);
        const size_t header = build_opt_tables(counts, quality, w, h, s, restart, &built, dst + 4);
        return code_frame(frame, restart, built, 4 + header, dst);
    }
    write_header(quality, w, h, dst + 4);
    dst[4 + kOffSofSampling] = sof_sampling(s);
    put16(dst + 4 + kOffDri + 4, restart);
    return code_frame(frame, restart, kHuff, kFrameData, dst);
}

}  // namespace

size_t encode_i420(const uint8_t* i420, int w, int h, int quality, int restart_mcus, uint8_t* dst) { return encode(i420, w, h, quality, k420, restart_mcus, false, dst); }
size_t encode_planes(const uint8_t* planes, int w, int h, int quality, Sampling s, uint8_t* dst) { return encode(planes, w, h, quality, s, restart_mcus(s), false, dst); }
size_t encode_planes_opt(const uint8_t* planes, int w, int h, int quality, Sampling s, uint8_t* dst) { return encode(planes, w, h, quality, s, restart_mcus(s), true, dst); }

// POPPY_FRAME_JPEG_SEQ / JPEG444_SEQ: three passes over the same coefficients — every frame counted into the sequence's sums (`copies` times), one table build,
// every frame coded on what it gave behind the one header
void encode_planes_seq(const uint8_t* planes, size_t frame_stride, int n, int copies, int w, int h, int quality, Sampling s, uint8_t* dst, size_t dst_stride) {
    const int restart = restart_mcus(s);
    std::vector<FrameBlocks> frames;
    for (int k = 0; k < n; ++k) frames.emplace_back(planes + (size_t)k * frame_stride, w, h, quality, s);
    SymbolCounts sums{};
    for (int k = 0; k < n; ++k) {
        SymbolCounts one{};
        count_frame(frames[k], restart, one);
        for (int t = 0; t < 4; ++t)
            for (int i = 0; i < table_symbols(t); ++i) table_of(sums, t)[i] += table_of(one, t)[i] * (uint32_t)copies;
    }
    HuffTables built{};
    uint8_t header[kHeaderBytes];
    const size_t header_bytes = build_opt_tables(sums, quality, w, h, s, restart, &built, header);
    for (int k = 0; k < n; ++k) {
        uint8_t* frame = dst + (size_t)k * dst_stride;
        memcpy(frame + 4, header, header_bytes);
        code_frame(frames[k], restart, built, 4 + header_bytes, frame);
    }
}

}  // namespace jpeg
}  // namespace poppy_hip

extern "C" {

size_t poppy_jpeg_frame_bytes(const uint8_t* frame) {
    return frame ? (size_t)frame[0] | (size_t)frame[1] << 8 | (size_t)frame[2] << 16 | (size_t)frame[3] << 24 : 0;
}

int poppy_i420_to_jpeg_frame(const uint8_t* i420, int width, int height, int quality, uint8_t* dst) {
    if (!i420 || !dst || width <= 0 || height <= 0 || quality < 1 || quality > 100) return POPPY_E_ARG;
    if (!jpeg_fits(width, height)) return POPPY_E_UNSUPPORTED;
    poppy_hip::jpeg::encode_planes(i420, width, height, quality, poppy_hip::jpeg::k420, dst);
    return POPPY_OK;
}

int poppy_i444_to_jpeg_frame(const uint8_t* i444, int width, int height, int quality, uint8_t* dst) {
    if (!i444 || !dst || width <= 0 || height <= 0 || quality < 1 || quality > 100) return POPPY_E_ARG;
    if (!jpeg_fits(width, height, poppy_hip::jpeg::k444)) return POPPY_E_UNSUPPORTED;
    poppy_hip::jpeg::encode_planes(i444, width, height, quality, poppy_hip::jpeg::k444, dst);
    return POPPY_OK;
}

int poppy_bgr_to_jpeg_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3 || quality < 1 || quality > 100) return POPPY_E_ARG;
    if (!jpeg_fits(width, height)) return POPPY_E_UNSUPPORTED;
    std::vector<uint8_t> i420(poppy_frame_bytes(POPPY_FRAME_I420, width, height));
    const int rc = poppy_bgr_to_i420(bgr, stride, width, height, i420.data());
    return rc ? rc : poppy_i420_to_jpeg_frame(i420.data(), width, height, quality, dst);
}

int poppy_bgr_to_jpeg444_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3 || quality < 1 || quality > 100) return POPPY_E_ARG;
    if (!jpeg_fits(width, height, poppy_hip::jpeg::k444)) return POPPY_E_UNSUPPORTED;
    std::vector<uint8_t> i444((size_t)width * height * 3);
    const int rc = poppy_bgr_to_i444(bgr, stride, width, height, i444.data());
    return rc ? rc : poppy_i444_to_jpeg_frame(i444.data(), width, height, quality, dst);
}

// The table rule of POPPY_FRAME_JPEG_OPT (include/poppy_hip.h states it step by step): T.81 Annex K.2 with every tie decided, lengths limited by K.3.
int poppy_jpeg_optimal_table(const uint32_t* counts, uint8_t* bits, uint8_t* vals, int* n_vals) {
    if (!counts || !bits || !vals || !n_vals) return POPPY_E_ARG;
    uint64_t freq[257], sum = 0;
    for (int i = 0; i < 256; ++i) { freq[i] = counts[i]; sum += counts[i]; }
    if (sum == 0 || sum >= 0xffffffffull) return POPPY_E_ARG;
    freq[256] = 1;                                          // the reserved entry: no real code is all ones
    int len[257] = {}, tree[257];                           // a symbol's code length so far, and the root of the tree it is in (the index that holds the tree's count)
    for (int i = 0; i <= 256; ++i) tree[i] = i;
    for (;;) {
        int c1 = -1, c2 = -1;                               // the smallest non-zero count, the largest index among equals; the same among the others
        for (int i = 0; i <= 256; ++i) if (freq[i] && (c1 < 0 || freq[i] <= freq[c1])) c1 = i;
        for (int i = 0; i <= 256; ++i) if (freq[i] && i != c1 && (c2 < 0 || freq[i] <= freq[c2])) c2 = i;
        if (c2 < 0) break;
        freq[c1] += freq[c2]; freq[c2] = 0;
        for (int i = 0; i <= 256; ++i) if (tree[i] == c1 || tree[i] == c2) { ++len[i]; tree[i] = c1; }
    }
    int of_length[258] = {};                                // lengths up to 256: 257 leaves
    for (int i = 0; i <= 256; ++i) if (len[i]) ++of_length[len[i]];
    for (int i = 256; i > 16; --i)                          // Annex K.3
        while (of_length[i] > 0) {
            int j = i - 2;
            while (of_length[j] == 0) --j;
            of_length[i] -= 2; of_length[i - 1] += 1; of_length[j + 1] += 2; of_length[j] -= 1;
        }
    int longest = 16;
    while (of_length[longest] == 0) --longest;
    --of_length[longest];                                   // the reserved entry
    for (int i = 0; i < 16; ++i) bits[i] = (uint8_t)of_length[i + 1];
    int n = 0;
    for (int l = 1; l <= 256; ++l)
        for (int i = 0; i < 256; ++i) if (len[i] == l) vals[n++] = (uint8_t)i;
    *n_vals = n;
    return POPPY_OK;
}

static int planes_to_jpeg_opt(const uint8_t* planes, int width, int height, int quality, poppy_hip::jpeg::Sampling s, uint8_t* dst) {
    if (!planes || !dst || width <= 0 || height <= 0 || quality < 1 || quality > 100) return POPPY_E_ARG;
    if (!jpeg_opt_fits(width, height, s)) return POPPY_E_UNSUPPORTED;
    poppy_hip::jpeg::encode_planes_opt(planes, width, height, quality, s, dst);
    return POPPY_OK;
}
int poppy_i420_to_jpeg_opt_frame(const uint8_t* i420, int width, int height, int quality, uint8_t* dst) { return planes_to_jpeg_opt(i420, width, height, quality, poppy_hip::jpeg::k420, dst); }
int poppy_i444_to_jpeg_opt_frame(const uint8_t* i444, int width, int height, int quality, uint8_t* dst) { return planes_to_jpeg_opt(i444, width, height, quality, poppy_hip::jpeg::k444, dst); }

int poppy_bgr_to_jpeg_opt_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3 || quality < 1 || quality > 100) return POPPY_E_ARG;
    if (!jpeg_opt_fits(width, height)) return POPPY_E_UNSUPPORTED;
    std::vector<uint8_t> i420(poppy_frame_bytes(POPPY_FRAME_I420, width, height));
    const int rc = poppy_bgr_to_i420(bgr, stride, width, height, i420.data());
    return rc ? rc : poppy_i420_to_jpeg_opt_frame(i420.data(), width, height, quality, dst);
}

int poppy_bgr_to_jpeg444_opt_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3 || quality < 1 || quality > 100) return POPPY_E_ARG;
    if (!jpeg_opt_fits(width, height, poppy_hip::jpeg::k444)) return POPPY_E_UNSUPPORTED;
    std::vector<uint8_t> i444((size_t)width * height * 3);
    const int rc = poppy_bgr_to_i444(bgr, stride, width, height, i444.data());
    return rc ? rc : poppy_i444_to_jpeg_opt_frame(i444.data(), width, height, quality, dst);
}

// POPPY_FRAME_JPEG_SEQ and POPPY_FRAME_JPEG444_SEQ (include/poppy_hip.h): the refusals, all from the arguments alone
static int jpeg_seq_refuses(const void* src, const void* dst, size_t frame_stride, size_t frame_bytes, int n_frames, int width, int height, int quality, poppy_hip::jpeg::Sampling s) {
    if (!src || !dst || n_frames < 1 || width <= 0 || height <= 0 || frame_stride < frame_bytes || quality < 1 || quality > 100) return POPPY_E_ARG;
    return jpeg_opt_fits(width, height, s) && jpeg_seq_fits(n_frames, width, height, s) ? POPPY_OK : POPPY_E_UNSUPPORTED;
}
static int planes_to_jpeg_seq(const uint8_t* planes, size_t frame_stride, int n_frames, int width, int height, int quality, poppy_hip::jpeg::Sampling s, uint8_t* dst) {
    const bool is444 = s == poppy_hip::jpeg::k444;
    if (width <= 0 || height <= 0) return POPPY_E_ARG;
    if (const int rc = jpeg_seq_refuses(planes, dst, frame_stride, raster_bytes(is444 ? kRasterI444 : kRasterI420, (size_t)width, (size_t)height), n_frames, width, height, quality, s)) return rc;
    poppy_hip::jpeg::encode_planes_seq(planes, frame_stride, n_frames, 1, width, height, quality, s, dst, (size_t)poppy_hip::jpeg::opt_frame_capacity((size_t)width, (size_t)height, s));
    return POPPY_OK;
}
int poppy_i420_frames_to_jpeg_seq_frames(const uint8_t* i420, size_t frame_stride, int n_frames, int width, int height, int quality, uint8_t* dst) {
    return planes_to_jpeg_seq(i420, frame_stride, n_frames, width, height, quality, poppy_hip::jpeg::k420, dst);
}
int poppy_i444_frames_to_jpeg_seq_frames(const uint8_t* i444, size_t frame_stride, int n_frames, int width, int height, int quality, uint8_t* dst) {
    return planes_to_jpeg_seq(i444, frame_stride, n_frames, width, height, quality, poppy_hip::jpeg::k444, dst);
}

static int bgr_frames_to_jpeg_seq(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality, poppy_hip::jpeg::Sampling s, uint8_t* dst) {
    if (width <= 0 || height <= 0 || stride < (size_t)width * 3) return POPPY_E_ARG;
    if (const int rc = jpeg_seq_refuses(bgr, dst, frame_stride, stride * ((size_t)height - 1) + (size_t)width * 3, n_frames, width, height, quality, s)) return rc;
    const bool is444 = s == poppy_hip::jpeg::k444;
    const size_t place = raster_bytes(is444 ? kRasterI444 : kRasterI420, (size_t)width, (size_t)height);
    std::vector<uint8_t> planes(place * (size_t)n_frames);
    for (int k = 0; k < n_frames; ++k)
        if (const int rc = (is444 ? poppy_bgr_to_i444 : poppy_bgr_to_i420)(bgr + (size_t)k * frame_stride, stride, width, height, planes.data() + (size_t)k * place)) return rc;
    return planes_to_jpeg_seq(planes.data(), place, n_frames, width, height, quality, s, dst);
}
int poppy_bgr_frames_to_jpeg_seq_frames(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality, uint8_t* dst) {
    return bgr_frames_to_jpeg_seq(bgr, stride, frame_stride, n_frames, width, height, quality, poppy_hip::jpeg::k420, dst);
}
int poppy_bgr_frames_to_jpeg444_seq_frames(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality, uint8_t* dst) {
    return bgr_frames_to_jpeg_seq(bgr, stride, frame_stride, n_frames, width, height, quality, poppy_hip::jpeg::k444, dst);
}

}  // extern "C"

// writer_image.h: a sequence that is n_copies times the same frame; that frame once in dst
int jpeg_seq_of_copies(const uint8_t* bgr, size_t stride, int n_copies, int width, int height, int quality, int format, uint8_t* dst) {
    const poppy_hip::jpeg::Sampling s = format == POPPY_FRAME_JPEG444_SEQ ? poppy_hip::jpeg::k444 : poppy_hip::jpeg::k420;
    if (width <= 0 || height <= 0 || stride < (size_t)width * 3) return POPPY_E_ARG;
    if (const int rc = jpeg_seq_refuses(bgr, dst, 0, 0, n_copies, width, height, quality, s)) return rc;
    std::vector<uint8_t> planes(raster_bytes(s == poppy_hip::jpeg::k444 ? kRasterI444 : kRasterI420, (size_t)width, (size_t)height));
    if (const int rc = (s == poppy_hip::jpeg::k444 ? poppy_bgr_to_i444 : poppy_bgr_to_i420)(bgr, stride, width, height, planes.data())) return rc;
    poppy_hip::jpeg::encode_planes_seq(planes.data(), 0, 1, n_copies, width, height, quality, s, dst, 0);
    return POPPY_OK;
}
