// jpeg_opt_host_check.cpp — the host statement of POPPY_FRAME_JPEG_OPT and POPPY_FRAME_JPEG444_OPT (poppy_amd/csrc/frame_jpeg.cpp) alone, on the host, under a
// sanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_opt_host_check.cpp poppy_amd/csrc/frame_jpeg.cpp \
//       poppy_amd/csrc/frame_sink.cpp poppy_amd/csrc/frame_gif.cpp poppy_amd/csrc/frame_pal8.cpp poppy_amd/csrc/frame_i444.cpp poppy_amd/csrc/frame_png.cpp \
//       poppy_amd/csrc/frame_png_runs.cpp -o /tmp/jpeg_opt_asan && /tmp/jpeg_opt_asan
// Every frame is coded into a heap buffer of EXACTLY poppy_frame_bytes(format, w, h) bytes from planes of exactly their own size, so a byte written behind the
// capacity or read behind a plane is the sanitizer's to report; so is a step of the table rule outside its arrays, which is why the rule also runs alone on the
// counts no small frame produces: 42 near-Fibonacci counts (an unlimited depth of 42, above libjpeg's 32 lengths), 256 equal counts, counts equal in pairs, a
// single symbol, sums at the limit.  Returns 0 when every `total` is inside its bounds, every frame ends with EOI, every table has a Kraft sum below 2^16 and
// every refusal is refused.
#include "../include/poppy_hip.h"
#include <cstdint>
#include <cstdio>
#include <vector>

static uint32_t g_state = 12345u;
static uint8_t noise() { g_state = g_state * 1664525u + 1013904223u; return (uint8_t)(g_state >> 24); }

// the rule on `counts`: POPPY_OK, as many values as counts, a Kraft sum that leaves the all-ones code free
static bool table_holds(const char* what, const std::vector<uint32_t>& counts) {
    std::vector<uint8_t> bits(16), vals(256);               // (heap: exactly the sizes the rule names)
    int n = -1, symbols = 0;
    const int rc = poppy_jpeg_optimal_table(counts.data(), bits.data(), vals.data(), &n);
    for (uint32_t c : counts) symbols += c != 0;
    unsigned long kraft = 0;
    int sum = 0;
    for (int l = 1; l <= 16; ++l) { kraft += (unsigned long)bits[l - 1] << (16 - l); sum += bits[l - 1]; }
    const bool ok = rc == POPPY_OK && n == symbols && sum == n && kraft < 65536;
    if (!ok) fprintf(stderr, "table %s: rc %d, %d values for %d symbols, Kraft sum %lu\n", what, rc, n, symbols, kraft);
    return ok;
}

int main() {
    int failures = 0, tables = 0;
    {
        std::vector<uint32_t> c(256, 0);
        c[0] = 1; c[1] = 2;
        for (int k = 2; k < 42; ++k) c[k] = c[k - 1] + c[k - 2] + 1;
        failures += !table_holds("near-Fibonacci", c); ++tables;
        std::vector<uint32_t> r(256, 0);
        for (int k = 0; k < 42; ++k) r[255 - k] = c[k];
        failures += !table_holds("near-Fibonacci, at the top", r); ++tables;
        failures += !table_holds("256 equal counts", std::vector<uint32_t>(256, 1)); ++tables;
        failures += !table_holds("256 large equal counts", std::vector<uint32_t>(256, 16000000)); ++tables;
        std::vector<uint32_t> p(256, 0);
        for (int k = 0; k < 256; ++k) p[k] = 3 + k / 2;
        failures += !table_holds("equal in pairs", p); ++tables;
        std::vector<uint32_t> one(256, 0);
        one[255] = 0xfffffffeu;
        failures += !table_holds("one symbol, the largest sum", one); ++tables;
        one[0] = 1; one[255] = 0xfffffffdu;
        failures += !table_holds("two symbols, the largest sum", one); ++tables;
        std::vector<uint32_t> steep(256, 0);
        for (int k = 0; k < 162; ++k) steep[k] = 1u << (k < 23 ? k : 23);
        failures += !table_holds("steep", steep); ++tables;
        for (int round = 0; round < 50; ++round) {
            std::vector<uint32_t> any(256, 0);
            for (int k = 0; k < 256; ++k) any[k] = noise() < 96 ? 0 : (uint32_t)noise() >> (noise() & 7);
            any[noise()] = 1;
            failures += !table_holds("random", any); ++tables;
        }
        std::vector<uint8_t> bits(16), vals(256);
        int n = 0;
        std::vector<uint32_t> zero(256, 0), full(256, 0);
        full[7] = 0xffffffffu;
        if (poppy_jpeg_optimal_table(zero.data(), bits.data(), vals.data(), &n) != POPPY_E_ARG || poppy_jpeg_optimal_table(full.data(), bits.data(), vals.data(), &n) != POPPY_E_ARG ||
            poppy_jpeg_optimal_table(nullptr, bits.data(), vals.data(), &n) != POPPY_E_ARG || poppy_jpeg_optimal_table(one.data(), bits.data(), vals.data(), nullptr) != POPPY_E_ARG) {
            fprintf(stderr, "a refusal of the table rule was not refused\n");
            ++failures;
        }
    }
    const int sizes[][2] = {{1, 1}, {2, 2}, {16, 16}, {17, 17}, {15, 33}, {48, 48}, {160, 128}, {16 * POPPY_JPEG_RESTART_MCUS + 1, 31}, {333, 211}};
    const int qualities[] = {100, 90, 10, 1};
    int frames = 0;
    size_t fullest = 0, fullest_cap = 1;
    for (const auto& wh : sizes) {
        const int w = wh[0], h = wh[1];
        for (int s444 = 0; s444 < 2; ++s444) {
            const int cw = s444 ? w : (w + 1) / 2, ch = s444 ? h : (h + 1) / 2, format = s444 ? POPPY_FRAME_JPEG444_OPT : POPPY_FRAME_JPEG_OPT;
            const size_t n = (size_t)w * h + 2 * (size_t)cw * ch, cap = poppy_frame_bytes(format, w, h);
            for (int content = 0; content < 5; ++content) {
                std::vector<uint8_t> planes(n);
                for (int p = 0; p < 3; ++p) {
                    const int pw = p ? cw : w, ph = p ? ch : h, s = p && !s444 ? 8 : 16;
                    uint8_t* plane = planes.data() + (p == 0 ? 0 : (size_t)w * h + (p == 2 ? (size_t)cw * ch : 0));
                    for (int y = 0; y < ph; ++y)
                        for (int x = 0; x < pw; ++x)
                            plane[(size_t)y * pw + x] = content == 0 ? noise() : content == 1 ? (uint8_t)(((x + y) & 1) * 255) : content == 2 ? 0 : content == 3 ? 255
                                                                                                                               : (uint8_t)((((x / s) + (y / s)) & 1) * 255);
                }
                for (int q : qualities) {
                    std::vector<uint8_t> frame(cap);
                    const int rc = (s444 ? poppy_i444_to_jpeg_opt_frame : poppy_i420_to_jpeg_opt_frame)(planes.data(), w, h, q, frame.data());
                    const size_t total = poppy_jpeg_frame_bytes(frame.data());
                    ++frames;
                    if (rc != POPPY_OK || total < 276 || total > cap || frame[total - 2] != 0xFF || frame[total - 1] != 0xD9) {
                        fprintf(stderr, "%d x %d (%s), content %d, quality %d: rc %d, total %zu of %zu\n", w, h, s444 ? "4:4:4" : "4:2:0", content, q, rc, total, cap);
                        ++failures;
                    }
                    if (total * fullest_cap > fullest * cap) { fullest = total; fullest_cap = cap; }
                }
            }
        }
    }
    // the BGR entries, from a frame with padded rows
    {
        const int w = 37, h = 21;
        const size_t stride = (size_t)w * 3 + 5;
        std::vector<uint8_t> bgr(stride * h - 5);                // (the last row has no padding behind it)
        for (uint8_t& b : bgr) b = noise();
        for (int s444 = 0; s444 < 2; ++s444) {
            const size_t cap = poppy_frame_bytes(s444 ? POPPY_FRAME_JPEG444_OPT : POPPY_FRAME_JPEG_OPT, w, h);
            std::vector<uint8_t> frame(cap);
            const int rc = (s444 ? poppy_bgr_to_jpeg444_opt_frame : poppy_bgr_to_jpeg_opt_frame)(bgr.data(), stride, w, h, 90, frame.data());
            const size_t total = poppy_jpeg_frame_bytes(frame.data());
            ++frames;
            if (rc != POPPY_OK || total < 276 || total > cap) { fprintf(stderr, "BGR entry %d: rc %d, total %zu of %zu\n", s444, rc, total, cap); ++failures; }
        }
    }
    printf("%d tables built, %d frames coded into buffers of exactly the capacity, %d failures; the fullest used %zu of %zu bytes\n", tables, frames, failures, fullest, fullest_cap);
    return failures ? 1 : 0;
}
