// jpeg_host_check.cpp — the host statement of POPPY_FRAME_JPEG (poppy_amd/csrc/frame_jpeg.cpp) alone, on the host, under a sanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_host_check.cpp poppy_amd/csrc/frame_jpeg.cpp \
//       poppy_amd/csrc/frame_sink.cpp poppy_amd/csrc/frame_gif.cpp poppy_amd/csrc/frame_pal8.cpp poppy_amd/csrc/frame_i444.cpp poppy_amd/csrc/frame_png.cpp \
//       -o /tmp/jpeg_asan && /tmp/jpeg_asan
// Every frame is coded into a heap buffer of EXACTLY poppy_frame_bytes(POPPY_FRAME_JPEG, w, h) bytes from an I420 frame of exactly its own size, so a byte
// written behind the capacity or read behind a plane is the sanitizer's to report.  The content is what stresses the capacity: noise at quality 100, saturated
// checkerboards, flat frames and the black / white MCU alternation, at sizes around one MCU and one restart interval.  Returns 0 when every `total` is inside
// its bounds and every frame ends with EOI.
#include "../include/poppy_hip.h"
#include <cstdint>
#include <cstdio>
#include <vector>

static uint32_t g_state = 12345u;
static uint8_t noise() { g_state = g_state * 1664525u + 1013904223u; return (uint8_t)(g_state >> 24); }

int main() {
    const int sizes[][2] = {{1, 1}, {2, 2}, {16, 16}, {17, 17}, {15, 33}, {48, 48}, {160, 128}, {16 * POPPY_JPEG_RESTART_MCUS + 1, 31}, {333, 211}};
    const int qualities[] = {100, 90, 10, 1};
    int failures = 0, frames = 0;
    size_t fullest = 0, fullest_cap = 1;
    for (const auto& wh : sizes) {
        const int w = wh[0], h = wh[1], cw = (w + 1) / 2, ch = (h + 1) / 2;
        const size_t n = poppy_frame_bytes(POPPY_FRAME_I420, w, h), cap = poppy_frame_bytes(POPPY_FRAME_JPEG, w, h);
        for (int content = 0; content < 5; ++content) {
            std::vector<uint8_t> i420(n);
            for (int p = 0; p < 3; ++p) {
                const int pw = p ? cw : w, ph = p ? ch : h, s = p ? 8 : 16;
                uint8_t* plane = i420.data() + (p == 0 ? 0 : (size_t)w * h + (p == 2 ? (size_t)cw * ch : 0));
                for (int y = 0; y < ph; ++y)
                    for (int x = 0; x < pw; ++x)
                        plane[(size_t)y * pw + x] = content == 0 ? noise() : content == 1 ? (uint8_t)(((x + y) & 1) * 255) : content == 2 ? 0 : content == 3 ? 255
                                                                                                                           : (uint8_t)((((x / s) + (y / s)) & 1) * 255);
            }
            for (int q : qualities) {
                std::vector<uint8_t> frame(cap);
                const int rc = poppy_i420_to_jpeg_frame(i420.data(), w, h, q, frame.data());
                const size_t total = poppy_jpeg_frame_bytes(frame.data());
                ++frames;
                if (rc != POPPY_OK || total < 617 + 3 || total > cap || frame[total - 2] != 0xFF || frame[total - 1] != 0xD9) {
                    fprintf(stderr, "%d x %d, content %d, quality %d: rc %d, total %zu of %zu\n", w, h, content, q, rc, total, cap);
                    ++failures;
                }
                if (total * fullest_cap > fullest * cap) { fullest = total; fullest_cap = cap; }
            }
        }
    }
    printf("%d frames coded into buffers of exactly the capacity, %d failures; the fullest used %zu of %zu bytes\n", frames, failures, fullest, fullest_cap);
    return failures ? 1 : 0;
}
