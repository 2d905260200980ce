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
void code_block_coefficients(const uint8_t* plane, int w, int h, int x0, int y0, const QualityTables& q, int table, int* zz) {
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
        zz[k] = f[n] < 0 ? -m : m;
    }
}

inline int category(int v) { int a = v < 0 ? -v : v, c = 0; while (a) { ++c; a >>= 1; } return c; }
inline void put_value(BitString& b, uint32_t huff, int v, int cat) {
    b.put(huff >> 8, (int)(huff & 255));
    if (cat) b.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1), cat);
}

void code_block(BitString& b, const int* zz, int* pred, int table) {
    const int diff = zz[0] - *pred;
    *pred = zz[0];
    const int dc_cat = category(diff);
    put_value(b, kHuff.dc[table][dc_cat], diff, dc_cat);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        if (zz[k] == 0) { ++run; continue; }
        for (; run >= 16; run -= 16) b.put(kHuff.ac[table][0xF0] >> 8, (int)(kHuff.ac[table][0xF0] & 255));
        const int cat = category(zz[k]);
        put_value(b, kHuff.ac[table][run << 4 | cat], zz[k], cat);
        run = 0;
    }
    if (run) b.put(kHuff.ac[table][0] >> 8, (int)(kHuff.ac[table][0] & 255));
}

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

// the frame of the planes of sampling `s` with restart intervals of `restart` MCUs (the header's DRI names it); returns `total`
size_t encode(const uint8_t* planes, int w, int h, int quality, Sampling s, int restart, uint8_t* dst) {
    const int side = mcu_side(s), mw = (w + side - 1) / side, mh = (h + side - 1) / side, n_mcu = mw * mh;
    const int cw = s == k444 ? w : (w + 1) / 2, ch = s == k444 ? h : (h + 1) / 2;      // the chroma planes
    const uint8_t *yp = planes, *up = yp + (size_t)w * h, *vp = up + (size_t)cw * ch;
    QualityTables q;
    fill_quality_tables(quality, &q);
    write_header(quality, w, h, dst + 4);
    dst[4 + kOffSofSampling] = sof_sampling(s);
    put16(dst + 4 + kOffDri + 4, restart);
    size_t at = kFrameData;
    int zz[64];
    for (int first = 0, seg = 0; first < n_mcu; first += restart, ++seg) {
        BitString b;
        int pred[3] = {0, 0, 0};
        for (int m = first; m < n_mcu && m < first + restart; ++m) {
            const int mx = m % mw, my = m / mw;
            for (int k = 0; k < (s == k444 ? 1 : 4); ++k) {       // the luma blocks: 2 x 2 of them in a 16 x 16 MCU, one in an 8 x 8 MCU
                code_block_coefficients(yp, w, h, side * mx + 8 * (k & 1), side * my + 8 * (k >> 1), q, 0, zz);
                code_block(b, zz, &pred[0], 0);
            }
            code_block_coefficients(up, cw, ch, 8 * mx, 8 * my, q, 1, zz);
            code_block(b, zz, &pred[1], 1);
            code_block_coefficients(vp, cw, ch, 8 * mx, 8 * my, q, 1, zz);
            code_block(b, zz, &pred[2], 1);
        }
        b.pad();
        for (uint8_t byte : b.bytes) { dst[at++] = byte; if (byte == 0xFF) dst[at++] = 0; }
        dst[at++] = 0xFF;
        dst[at++] = first + restart < n_mcu ? (uint8_t)(0xD0 + (seg & 7)) : (uint8_t)0xD9;
    }
    dst[0] = (uint8_t)at; dst[1] = (uint8_t)(at >> 8); dst[2] = (uint8_t)(at >> 16); dst[3] = (uint8_t)(at >> 24);
    return at;
}

}  // namespace

size_t encode_i420(const uint8_t* i420, int w, int h, int quality, int restart_mcus, uint8_t* dst) { return encode(i420, w, h, quality, k420, restart_mcus, dst); }
size_t encode_planes(const uint8_t* planes, int w, int h, int quality, Sampling s, uint8_t* dst) { return encode(planes, w, h, quality, s, restart_mcus(s), dst); }

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

}  // extern "C"
