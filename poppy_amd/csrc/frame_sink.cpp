// frame_sink.cpp — file sinks for the frame hand-off ("optional raw/PPM/Y4M sink"): the reference writes through
// cv::VideoWriter (FFV1, src/poppy.cpp:249), which needs a codec library; these need none.  Host only, no GPU involved:
// poppy_sink_write has the poppy_write_cb signature, so a sink plugs straight into poppy_hip_morph / poppy_hip_morph_frames.
//   POPPY_SINK_RAW   one file, frames back to back, width*3 bytes per row, BGR (what the writer callback receives)
//   POPPY_SINK_PPM   one binary PPM (P6, RGB) per frame; the path holds exactly one %d / %<width>d / %0<width>d (frame index from 0)
//   POPPY_SINK_Y4M   one YUV4MPEG2 file, C444, full-range BT.601 in 8-bit integer arithmetic (lossless containers downstream can
//                    re-encode it; the conversion is this file's, not the reference's)
//   POPPY_SINK_Y4M420  one YUV4MPEG2 file, C420jpeg, that takes I420 frames as they are (poppy_hip_set_frame_format)
//   POPPY_SINK_GIF   one animated GIF89a file that takes PAL8 frames as they are: a local colour table and one LZW image per frame
//   POPPY_SINK_GIF_GLOBAL  the same for PAL8_SEQ frames: the first frame's palette as the global colour table, local tables only where a frame's palette differs
//   POPPY_SINK_GIF_CODED   POPPY_SINK_GIF's file from POPPY_FRAME_GIF frames, whose image data arrives coded (frame_gif.cpp, kernels_frame_gif.hip): nothing is coded here
//   POPPY_SINK_GIF_GLOBAL_CODED  POPPY_SINK_GIF_GLOBAL's file from coded frames (POPPY_FRAME_GIF_SEQ): the first frame's palette as the global table, local tables only where a palette differs
//   POPPY_SINK_MJPEG  one RIFF AVI file, a `vids` / `MJPG` stream, from POPPY_FRAME_JPEG and POPPY_FRAME_JPEG444 frames and their OPT forms, whose bytes arrive coded (frame_jpeg.cpp, kernels_frame_jpeg.hip)
//   POPPY_SINK_PNG   one PNG file per frame from POPPY_FRAME_PNG, POPPY_FRAME_PNG_RUNS, POPPY_FRAME_PNG_OPT and POPPY_FRAME_PNG_SEQ frames, whose bytes arrive coded (frame_png.cpp, frame_png_runs.cpp, frame_png_opt.cpp, frame_png_seq.cpp, kernels_frame_png.hip); the path as under PPM
// and the library's definition of the I420 hand-off format: poppy_bgr_to_i420 (kernels_frame_format.hip computes the same bytes on the device).
#include "frame_limits.h"
#include "gif_lzw.h"
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct poppy_sink {
    int format = 0, w = 0, h = 0, frames = 0;
    bool failed = false;
    std::string path;                  // PPM, PNG: the text before the pattern's conversion
    std::string tail;                  // PPM, PNG: the text after it
    int pad = 0; bool zero = false;    // PPM, PNG: width and zero flag of the conversion (%d, %5d, %05d)
    FILE* f = nullptr;
    std::vector<uint8_t> row;
    int delay_cs = 3;                  // GIF: the frames' delay in centiseconds
    bool head_written = false;         // GIF_GLOBAL: the header waits for the first frame's palette
    uint8_t global_pal[768];           // ... which is the global colour table
    int fps_num = 30, fps_den = 1;     // MJPEG: the stream's rate and scale
    uint64_t at = 0;                   // MJPEG: the file's length so far
    uint32_t largest = 0;              // MJPEG: the largest chunk's payload
    std::vector<uint32_t> index;       // MJPEG: per frame the chunk's offset from the `movi` fourcc and its length
};

namespace {

// One image's LZW data: the coder of gif_lzw.h (codes, width growth and the restart of a full table are stated there), closed by the end code; the packed bits go
// out in sub-blocks of at most 255 bytes, then the block terminator.
struct GifLzw {
    FILE* f;
    bool ok = true;
    uint8_t block[255]; int n_block = 0;
    poppy_hip::GifLzwCoder coder;
    explicit GifLzw(FILE* file) : f(file) {}
    void flush_block() {
        if (!n_block) return;
        const uint8_t len = (uint8_t)n_block;
        if (fwrite(&len, 1, 1, f) != 1 || fwrite(block, 1, (size_t)n_block, f) != (size_t)n_block) ok = false;
        n_block = 0;
    }
    void operator()(uint8_t byte) { block[n_block++] = byte; if (n_block == 255) flush_block(); }
    void encode(const uint8_t* px, size_t n) {
        const int width = coder.run(px, n, *this);
        coder.put(poppy_hip::GifLzwCoder::kEnd, width, *this);
        coder.flush(*this);
        flush_block();
        const uint8_t zero = 0;
        if (fwrite(&zero, 1, 1, f) != 1) ok = false;         // the block terminator
    }
};

// header, logical screen (with `global` as its 256-entry colour table, or without one), the NETSCAPE2.0 application block: loop for ever
bool gif_head(poppy_sink* s, const uint8_t* global) {
    const int width = s->w, height = s->h;
    const uint8_t head[13] = {'G', 'I', 'F', '8', '9', 'a', (uint8_t)(width & 255), (uint8_t)(width >> 8), (uint8_t)(height & 255), (uint8_t)(height >> 8), (uint8_t)(global ? 0xF7 : 0x70), 0, 0};
    const uint8_t loop[19] = {0x21, 0xFF, 11, 'N', 'E', 'T', 'S', 'C', 'A', 'P', 'E', '2', '.', '0', 3, 1, 0, 0, 0};
    s->head_written = true;
    return fwrite(head, 1, 13, s->f) == 13 && (!global || fwrite(global, 1, 768, s->f) == 768) && fwrite(loop, 1, 19, s->f) == 19;
}

bool gif_frame(poppy_sink* s, const uint8_t* pal8) {
    const int w = s->w, h = s->h;
    const size_t n = (size_t)w * h;
    bool local = true;
    if (s->format == POPPY_SINK_GIF_GLOBAL) {
        if (!s->head_written) { memcpy(s->global_pal, pal8 + n, 768); if (!gif_head(s, s->global_pal)) return false; }
        local = memcmp(s->global_pal, pal8 + n, 768) != 0;
    }
    const uint8_t gce[8] = {0x21, 0xF9, 4, 0, (uint8_t)(s->delay_cs & 255), (uint8_t)(s->delay_cs >> 8), 0, 0};
    const uint8_t desc[10] = {0x2C, 0, 0, 0, 0, (uint8_t)(w & 255), (uint8_t)(w >> 8), (uint8_t)(h & 255), (uint8_t)(h >> 8), (uint8_t)(local ? 0x87 : 0x00)};      // local table, 256 entries, or none
    const uint8_t min_code = 8;
    if (fwrite(gce, 1, 8, s->f) != 8 || fwrite(desc, 1, 10, s->f) != 10 || (local && fwrite(pal8 + n, 1, 768, s->f) != 768) || fwrite(&min_code, 1, 1, s->f) != 1) return false;
    GifLzw z(s->f);
    z.encode(pal8, n);
    return z.ok;
}

// whether the sink writes GIF89a, and whether its frames arrive coded (stride 0)
bool sink_is_gif(int format) { return format == POPPY_SINK_GIF || format == POPPY_SINK_GIF_GLOBAL || format == POPPY_SINK_GIF_CODED || format == POPPY_SINK_GIF_GLOBAL_CODED; }
bool sink_takes_coded(int format) { return format == POPPY_SINK_GIF_CODED || format == POPPY_SINK_GIF_GLOBAL_CODED; }
bool sink_has_global_table(int format) { return format == POPPY_SINK_GIF_GLOBAL || format == POPPY_SINK_GIF_GLOBAL_CODED; }

// a coded frame (POPPY_FRAME_GIF, POPPY_FRAME_GIF_SEQ): the palette as the local table — GIF_GLOBAL_CODED: only where it differs from the global table, which is
// the first frame's —, then the frame's image data as it is
bool gif_coded_frame(poppy_sink* s, const uint8_t* frame) {
    const int w = s->w, h = s->h;
    const size_t total = poppy_gif_frame_bytes(frame);
    // (772 + 3 is not coded_length_ok's bound, the smallest frame a coder gives, but one byte less: what keeps the two reads here, frame[772] and frame[total - 1],
    // apart and inside the frame.  The sink has always taken such a frame from a caller; it goes on doing so.)
    if (total < 772 + 3 || total > poppy_frame_bytes(POPPY_FRAME_GIF, w, h) || frame[772] != 8 || frame[total - 1] != 0) return false;
    bool local = true;
    if (sink_has_global_table(s->format)) {
        if (!s->head_written) { memcpy(s->global_pal, frame + 4, 768); if (!gif_head(s, s->global_pal)) return false; }
        local = memcmp(s->global_pal, frame + 4, 768) != 0;
    }
    const uint8_t gce[8] = {0x21, 0xF9, 4, 0, (uint8_t)(s->delay_cs & 255), (uint8_t)(s->delay_cs >> 8), 0, 0};
    const uint8_t desc[10] = {0x2C, 0, 0, 0, 0, (uint8_t)(w & 255), (uint8_t)(w >> 8), (uint8_t)(h & 255), (uint8_t)(h >> 8), (uint8_t)(local ? 0x87 : 0x00)};
    const size_t from = local ? 4 : 772;
    return fwrite(gce, 1, 8, s->f) == 8 && fwrite(desc, 1, 10, s->f) == 10 && fwrite(frame + from, 1, total - from, s->f) == total - from;
}

// ---- POPPY_SINK_MJPEG: a RIFF AVI with one Motion-JPEG video stream (include/poppy_hip.h names every chunk) ----
// Frames under a byte budget (poppy_hip_set_jpeg_budget) need nothing of their own here: every frame is a complete file with its own DQT, the sink reads SOF0 and
// `total` and never DQT, so frames of differing qualities stand side by side in one stream (tests/test_host_jpeg_budget.py writes such a file).
constexpr long kAviMovi = 220;                              // the file offset of the `movi` fourcc; the first chunk follows it
constexpr long kAviRiffSize = 4, kAviTotalFrames = 48, kAviBuffer = 60, kAviLength = 140, kAviStreamBuffer = 144, kAviMoviSize = 216;

void le32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

bool avi_head(poppy_sink* s) {
    uint8_t h[224];
    memset(h, 0, sizeof h);
    auto tag = [&](int at, const char* t) { memcpy(h + at, t, 4); };
    const uint32_t w = (uint32_t)s->w, ht = (uint32_t)s->h;
    tag(0, "RIFF"); tag(8, "AVI ");
    tag(12, "LIST"); le32(h + 16, 192); tag(20, "hdrl");
    tag(24, "avih"); le32(h + 28, 56);
    le32(h + 32, (uint32_t)((1000000ll * s->fps_den + s->fps_num / 2) / s->fps_num));      // dwMicroSecPerFrame
    le32(h + 44, 0x10);                                     // AVIF_HASINDEX
    le32(h + 56, 1);                                        // dwStreams
    le32(h + 64, w); le32(h + 68, ht);
    tag(88, "LIST"); le32(h + 92, 116); tag(96, "strl");
    tag(100, "strh"); le32(h + 104, 56); tag(108, "vids"); tag(112, "MJPG");
    le32(h + 128, (uint32_t)s->fps_den); le32(h + 132, (uint32_t)s->fps_num);      // dwScale, dwRate
    le32(h + 148, 0xffffffffu);                             // dwQuality: the default
    h[160] = (uint8_t)w; h[161] = (uint8_t)(w >> 8); h[162] = (uint8_t)ht; h[163] = (uint8_t)(ht >> 8);      // rcFrame's right and bottom
    tag(164, "strf"); le32(h + 168, 40);
    le32(h + 172, 40); le32(h + 176, w); le32(h + 180, ht); h[184] = 1; h[186] = 24; tag(188, "MJPG"); le32(h + 192, w * ht * 3);
    tag(212, "LIST"); tag(220, "movi");
    s->at = sizeof h;
    return fwrite(h, 1, sizeof h, s->f) == sizeof h;
}

// the width and height that the file's SOF0 names, and component 1's sampling byte (a walk over the marker segments in front of SOS, inside n bytes); false when there is none
bool jpeg_sof0_size(const uint8_t* jfif, size_t n, int* w, int* h, int* sampling) {
    size_t at = 2;
    while (at + 4 <= n && jfif[at] == 0xFF) {
        const int marker = jfif[at + 1];
        const size_t len = (size_t)jfif[at + 2] << 8 | jfif[at + 3];
        if (marker == 0xDA || len < 2 || at + 2 + len > n) return false;
        if (marker == 0xC0) {
            if (len < 10) return false;
            *h = jfif[at + 5] << 8 | jfif[at + 6]; *w = jfif[at + 7] << 8 | jfif[at + 8]; *sampling = jfif[at + 11];
            return true;
        }
        at += 2 + len;
    }
    return false;
}

// whether the file's first DHT segment in front of SOS is, byte for byte, the fixed header's with the four Annex K tables (a file without one: yes — it is held
// as every frame was before there were per-frame tables)
bool jpeg_dht_is_standard(const uint8_t* jfif, size_t n) {
    using namespace poppy_hip::jpeg;
    size_t at = 2;
    while (at + 4 <= n && jfif[at] == 0xFF) {
        const int marker = jfif[at + 1];
        const size_t len = (size_t)jfif[at + 2] << 8 | jfif[at + 3];
        if (marker == 0xDA || len < 2 || at + 2 + len > n) return true;
        if (marker == 0xC4) {
            static const std::array<uint8_t, kOffDri - kOffDht> standard = [] {      // the fixed header's DHT segment with its marker (no quality or size changes it): built once
                uint8_t fixed[kHeaderBytes];
                write_header(POPPY_JPEG_QUALITY_DEFAULT, 1, 1, fixed);
                std::array<uint8_t, kOffDri - kOffDht> dht;
                memcpy(dht.data(), fixed + kOffDht, dht.size());
                return dht;
            }();
            return 2 + len == standard.size() && memcmp(jfif + at, standard.data(), standard.size()) == 0;
        }
        at += 2 + len;
    }
    return true;
}

bool mjpeg_frame(poppy_sink* s, const uint8_t* frame) {
    const size_t total = poppy_jpeg_frame_bytes(frame);
    const size_t cap420 = poppy_frame_bytes(POPPY_FRAME_JPEG, s->w, s->h);
    if (total < 4 + 4 || total > poppy_frame_bytes(POPPY_FRAME_JPEG444_OPT, s->w, s->h)) return false;      // (the largest of the four capacities)
    const uint8_t* jfif = frame + 4;
    const size_t n = total - 4, pad = n & 1;
    int w = 0, h = 0, sampling = 0;
    // (the header is read inside the smaller capacity, which every frame's buffer has)
    if (jfif[0] != 0xFF || jfif[1] != 0xD8 || !jpeg_sof0_size(jfif, n < cap420 - 4 ? n : cap420 - 4, &w, &h, &sampling) || w != s->w || h != s->h) return false;
    // a 4:4:4 frame is held to its own capacity, and a frame on tables of its own (POPPY_FRAME_JPEG_OPT, POPPY_FRAME_JPEG444_OPT) to the OPT capacity of its sampling
    const bool opt = !jpeg_dht_is_standard(jfif, n < cap420 - 4 ? n : cap420 - 4);
    const int held_as = sampling == 0x11 ? (opt ? POPPY_FRAME_JPEG444_OPT : POPPY_FRAME_JPEG444) : (opt ? POPPY_FRAME_JPEG_OPT : POPPY_FRAME_JPEG);
    if (total > poppy_frame_bytes(held_as, s->w, s->h)) return false;
    // the file with this chunk, the index's chunk header and every index entry stays below 4 GiB
    if (s->at + 8 + n + pad + 8 + 16 * (uint64_t)(s->index.size() / 2 + 1) > 0xffffffffull) return false;
    uint8_t head[8] = {'0', '0', 'd', 'c'};
    le32(head + 4, (uint32_t)n);
    const uint8_t zero = 0;
    if (fwrite(head, 1, 8, s->f) != 8 || fwrite(jfif, 1, n, s->f) != n || (pad && fwrite(&zero, 1, 1, s->f) != 1)) return false;
    s->index.push_back((uint32_t)(s->at - kAviMovi)); s->index.push_back((uint32_t)n);
    s->at += 8 + n + pad;
    if (n > s->largest) s->largest = (uint32_t)n;
    return true;
}

// the name of the sink's next numbered file (PPM, PNG)
std::string numbered_name(const poppy_sink* s) {
    std::string num = std::to_string(s->frames);
    if ((int)num.size() < s->pad) num.insert(0, (size_t)s->pad - num.size(), s->zero ? '0' : ' ');
    return s->path + num + s->tail;
}

// a POPPY_FRAME_PNG, POPPY_FRAME_PNG_RUNS, POPPY_FRAME_PNG_OPT or POPPY_FRAME_PNG_SEQ frame (the file does not say which: `total` is held to the larger capacity; PNG_OPT's and PNG_SEQ's are PNG_RUNS'): its bytes 4 .. total as one file, once
// the signature, IHDR's size and `total` are what the sink's size allows
bool png_frame(poppy_sink* s, const uint8_t* frame) {
    using namespace poppy_hip::png;
    const size_t total = poppy_png_frame_bytes(frame);
    if (total < kFrameMinBytes || total > std::max(poppy_frame_bytes(POPPY_FRAME_PNG, s->w, s->h), poppy_frame_bytes(POPPY_FRAME_PNG_RUNS, s->w, s->h)) || memcmp(frame + kOffSignature, kSignature, 8) != 0) return false;
    const uint8_t* ihdr = frame + kOffIhdr;
    const uint32_t w = (uint32_t)ihdr[8] << 24 | (uint32_t)ihdr[9] << 16 | (uint32_t)ihdr[10] << 8 | ihdr[11], h = (uint32_t)ihdr[12] << 24 | (uint32_t)ihdr[13] << 16 | (uint32_t)ihdr[14] << 8 | ihdr[15];
    if (memcmp(ihdr + 4, "IHDR", 4) != 0 || w != (uint32_t)s->w || h != (uint32_t)s->h) return false;
    FILE* f = fopen(numbered_name(s).c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(frame + 4, 1, total - 4, f) == total - 4;
    return fclose(f) == 0 && ok;
}

// the index behind the last chunk, then the lengths and counts that were not known at the head
bool avi_close(poppy_sink* s) {
    const uint32_t frames = (uint32_t)(s->index.size() / 2);
    std::vector<uint8_t> idx(8 + 16 * (size_t)frames);
    memcpy(idx.data(), "idx1", 4); le32(idx.data() + 4, 16 * frames);
    for (uint32_t k = 0; k < frames; ++k) {
        uint8_t* e = idx.data() + 8 + 16 * (size_t)k;
        memcpy(e, "00dc", 4); le32(e + 4, 0x10); le32(e + 8, s->index[2 * k]); le32(e + 12, s->index[2 * k + 1]);      // AVIIF_KEYFRAME
    }
    if (fwrite(idx.data(), 1, idx.size(), s->f) != idx.size()) return false;
    const uint64_t end = s->at + idx.size();
    const struct { long at; uint32_t v; } patch[] = {{kAviRiffSize, (uint32_t)(end - 8)}, {kAviTotalFrames, frames}, {kAviBuffer, s->largest}, {kAviLength, frames},
                                                     {kAviStreamBuffer, s->largest}, {kAviMoviSize, (uint32_t)(s->at - kAviMovi)}};
    for (const auto& p : patch) {
        uint8_t v[4]; le32(v, p.v);
        if (fseek(s->f, p.at, SEEK_SET) != 0 || fwrite(v, 1, 4, s->f) != 4) return false;
    }
    return true;
}

}  // namespace

extern "C" {

size_t poppy_frame_bytes(int format, int width, int height) {
    const FormatTraits* t = format_traits(format);                 // (frame_limits.h: the format's record)
    return t && width > 0 && height > 0 ? frame_bytes(*t, width, height) : 0;
}

// Y: the C444 branch of poppy_sink_write.  U, V of each 2 x 2 block (n = 1, 2 or 4 pixels at the right and bottom edges, k = log2 n) from
// the block's channel sums with the same coefficients: ((c_r * sum R + c_g * sum G + c_b * sum B + (32768 << k)) >> (16 + k)) + 128, clamped.
int poppy_bgr_to_i420(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3) return POPPY_E_ARG;
    const int cw = (width + 1) / 2, ch = (height + 1) / 2;
    auto clamp = [](int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); };
    for (int y = 0; y < height; ++y) {
        const uint8_t* p = bgr + (size_t)y * stride;
        uint8_t* o = dst + (size_t)y * width;
        for (int x = 0; x < width; ++x) o[x] = clamp((19595 * p[3 * x + 2] + 38470 * p[3 * x + 1] + 7471 * p[3 * x] + 32768) >> 16);
    }
    uint8_t* u = dst + (size_t)width * height;
    uint8_t* v = u + (size_t)cw * ch;
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const int nx = 2 * cx + 1 < width ? 2 : 1, ny = 2 * cy + 1 < height ? 2 : 1, k = (nx >> 1) + (ny >> 1);
            int sb = 0, sg = 0, sr = 0;
            for (int r = 0; r < ny; ++r)
                for (int q = 0; q < nx; ++q) {
                    const uint8_t* px = bgr + (size_t)(2 * cy + r) * stride + (size_t)(2 * cx + q) * 3;
                    sb += px[0]; sg += px[1]; sr += px[2];
                }
            u[(size_t)cy * cw + cx] = clamp(((-11059 * sr - 21709 * sg + 32768 * sb + (32768 << k)) >> (16 + k)) + 128);
            v[(size_t)cy * cw + cx] = clamp(((32768 * sr - 27439 * sg - 5329 * sb + (32768 << k)) >> (16 + k)) + 128);
        }
    return POPPY_OK;
}

poppy_sink* poppy_sink_open(const char* path, int format, int width, int height, int fps_num, int fps_den) {
    if (!path || width <= 0 || height <= 0 || (!sink_is_gif(format) && format != POPPY_SINK_MJPEG && format != POPPY_SINK_PNG && (format < POPPY_SINK_RAW || format > POPPY_SINK_Y4M420))) return nullptr;
    poppy_sink* s = new poppy_sink();
    s->format = format; s->w = width; s->h = height; s->path = path;
    if (format == POPPY_SINK_PPM || format == POPPY_SINK_PNG) {
        // The pattern is parsed here, never handed to printf: exactly one conversion of the form %d / %<width>d / %0<width>d ("%%" is a
        // literal percent sign); anything else — %s, %n, a second conversion, no conversion at all (every frame would overwrite the
        // same file) — is refused.
        std::string head, tail;
        bool seen = false, bad = false;
        const std::string pat = path;
        for (size_t i = 0; i < pat.size() && !bad; ++i) {
            if (pat[i] != '%') { (seen ? tail : head) += pat[i]; continue; }
            if (i + 1 < pat.size() && pat[i + 1] == '%') { (seen ? tail : head) += '%'; ++i; continue; }
            if (seen) { bad = true; break; }
            size_t j = i + 1;
            if (j < pat.size() && pat[j] == '0') { s->zero = true; ++j; }
            int wdt = 0;
            while (j < pat.size() && pat[j] >= '0' && pat[j] <= '9' && wdt < 100) wdt = wdt * 10 + (pat[j++] - '0');
            if (j >= pat.size() || pat[j] != 'd' || wdt > 20) { bad = true; break; }
            s->pad = wdt; seen = true; i = j;
        }
        if (bad || !seen) { delete s; return nullptr; }
        s->path = head; s->tail = tail;
    }
    if ((sink_is_gif(format) || format == POPPY_SINK_MJPEG) && (width > 65535 || height > 65535)) { s->failed = true; return s; }      // GIF's 16-bit screen, JPEG's 16-bit SOF0: every write fails, close says so
    if (format == POPPY_SINK_PNG && !png_fits(width, height) && !png_runs_fits(width, height)) { s->failed = true; return s; }      // no such frame: every write fails, close says so
    if (format != POPPY_SINK_PPM && format != POPPY_SINK_PNG) {
        s->f = fopen(path, "wb");
        if (!s->f) { delete s; return nullptr; }
        if (format == POPPY_SINK_Y4M)
            fprintf(s->f, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C444 XCOLORRANGE=FULL\n", width, height, fps_num > 0 ? fps_num : 30, fps_den > 0 ? fps_den : 1);
        else if (format == POPPY_SINK_Y4M420)
            fprintf(s->f, "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=FULL\n", width, height, fps_num > 0 ? fps_num : 30, fps_den > 0 ? fps_den : 1);
        else if (sink_is_gif(format)) {
            const long long num = fps_num > 0 ? fps_num : 30, den = fps_den > 0 ? fps_den : 1;
            const long long cs = (den * 100 + num / 2) / num;
            s->delay_cs = (int)(cs < 1 ? 1 : cs > 65535 ? 65535 : cs);
            if (!sink_has_global_table(format) && !gif_head(s, nullptr)) s->failed = true;      // (a global table: with the first frame)
        } else if (format == POPPY_SINK_MJPEG) {
            s->fps_num = fps_num > 0 ? fps_num : 30; s->fps_den = fps_den > 0 ? fps_den : 1;
            if (!avi_head(s)) s->failed = true;
        }
    }
    s->row.resize((size_t)width * 3);
    return s;
}

void poppy_sink_write(void* user, const uint8_t* bgr, int width, int height, size_t stride) {
    poppy_sink* s = (poppy_sink*)user;
    if (!s || s->failed) return;
    // (an I420 frame comes with stride == width: the BGR sinks refuse it, and the I420 sink refuses anything else)
    // (a coded frame comes with stride == 0: every other sink refuses it below, and the coded sinks refuse anything else)
    if (s->format == POPPY_SINK_MJPEG) {
        if (!bgr || width != s->w || height != s->h || stride != 0 || !mjpeg_frame(s, bgr)) s->failed = true; else ++s->frames;
        return;
    }
    if (s->format == POPPY_SINK_PNG) {
        if (!bgr || width != s->w || height != s->h || stride != 0 || !png_frame(s, bgr)) s->failed = true; else ++s->frames;
        return;
    }
    if (sink_takes_coded(s->format)) {
        if (!bgr || width != s->w || height != s->h || stride != 0 || !gif_coded_frame(s, bgr)) s->failed = true; else ++s->frames;
        return;
    }
    const bool i420 = s->format == POPPY_SINK_Y4M420, pal8 = s->format == POPPY_SINK_GIF || s->format == POPPY_SINK_GIF_GLOBAL;
    if (!bgr || width != s->w || height != s->h || ((i420 || pal8) ? stride != (size_t)width : stride < (size_t)width * 3)) { s->failed = true; return; }
    FILE* f = s->f;
    if (pal8) {
        if (!gif_frame(s, bgr)) s->failed = true; else ++s->frames;
        return;
    }
    if (i420) {
        const size_t n = poppy_frame_bytes(POPPY_FRAME_I420, width, height);
        if (fputs("FRAME\n", f) < 0 || fwrite(bgr, 1, n, f) != n) s->failed = true; else ++s->frames;
        return;
    }
    if (s->format == POPPY_SINK_PPM) {
        f = fopen(numbered_name(s).c_str(), "wb");
        if (!f) { s->failed = true; return; }
        fprintf(f, "P6\n%d %d\n255\n", width, height);
    } else if (s->format == POPPY_SINK_Y4M) {
        fputs("FRAME\n", f);
    }
    bool ok = true;
    if (s->format == POPPY_SINK_RAW) {
        for (int y = 0; y < height && ok; ++y) ok = fwrite(bgr + (size_t)y * stride, 1, (size_t)width * 3, f) == (size_t)width * 3;
    } else if (s->format == POPPY_SINK_PPM) {
        for (int y = 0; y < height && ok; ++y) {
            const uint8_t* p = bgr + (size_t)y * stride;
            for (int x = 0; x < width; ++x) { s->row[3 * x] = p[3 * x + 2]; s->row[3 * x + 1] = p[3 * x + 1]; s->row[3 * x + 2] = p[3 * x]; }
            ok = fwrite(s->row.data(), 1, (size_t)width * 3, f) == (size_t)width * 3;
        }
        fclose(f);
    } else {
        // planar Y, U, V; JFIF full-range BT.601 with 16 fractional bits: Y = 0.299 R + 0.587 G + 0.114 B, U = 128 - 0.168736 R - 0.331264 G + 0.5 B, ...
        for (int plane = 0; plane < 3 && ok; ++plane)
            for (int y = 0; y < height && ok; ++y) {
                const uint8_t* p = bgr + (size_t)y * stride;
                for (int x = 0; x < width; ++x) {
                    const int b = p[3 * x], g = p[3 * x + 1], r = p[3 * x + 2];
                    int v;
                    if (plane == 0) v = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
                    else if (plane == 1) v = ((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128;
                    else v = ((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128;
                    s->row[x] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
                }
                ok = fwrite(s->row.data(), 1, (size_t)width, f) == (size_t)width;
            }
    }
    if (!ok) s->failed = true; else ++s->frames;
}

int poppy_sink_close(poppy_sink* s) {
    if (!s) return POPPY_E_ARG;
    if (s->f && sink_has_global_table(s->format) && !s->failed && !s->head_written && !gif_head(s, nullptr)) s->failed = true;      // no frame came: GIF's empty file
    if (s->f && sink_is_gif(s->format) && !s->failed && fputc(0x3B, s->f) == EOF) s->failed = true;      // the trailer
    if (s->f && s->format == POPPY_SINK_MJPEG && !s->failed && !avi_close(s)) s->failed = true;
    const int n = s->failed ? POPPY_E_DEVICE : s->frames;
    if (s->f) fclose(s->f);
    delete s;
    return n;
}

}  // extern "C"
