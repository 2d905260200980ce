// jpeg_seq_budget_host_check.cpp — the host statements of the JPEG sequence budget (poppy_amd/csrc/frame_jpeg_seq_budget.cpp over frame_jpeg.cpp's coder) alone, on
// the host, under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_seq_budget_host_check.cpp poppy_amd/csrc/frame_jpeg_seq_budget.cpp \
//       poppy_amd/csrc/frame_jpeg_budget.cpp poppy_amd/csrc/frame_jpeg.cpp poppy_amd/csrc/frame_i444.cpp poppy_amd/csrc/frame_sink.cpp poppy_amd/csrc/frame_gif.cpp \
//       poppy_amd/csrc/frame_pal8.cpp poppy_amd/csrc/frame_png.cpp poppy_amd/csrc/frame_png_runs.cpp poppy_amd/csrc/frame_png_opt.cpp poppy_amd/csrc/frame_png_seq.cpp \
//       -o /tmp/jpeg_seq_budget_asan && /tmp/jpeg_seq_budget_asan
// BGR frames with padded rows and padded frames, planes and every frame's destination lie in heap buffers of EXACTLY their size, so a byte read or written beside
// them is the sanitizer's to report.  Sequences of 1, 2 and 5 frames of noise, saturated noise and flat frames, both samplings; the table of the 100 summed sizes
// from the fixed-quality statement, then per budget (one above 2^32 among them): the statement's quality is the search's on the summed table, every frame is the
// fixed-quality frame at it, and the files fit together unless the quality is 1.  The refusals last.  Returns 0 when every call returns what the rule promises.
#include "../include/poppy_hip.h"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

static uint32_t g_state = 2463534242u;
static uint32_t next() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

using Bytes = std::unique_ptr<uint8_t[]>;
static Bytes exact(size_t n) { return Bytes(new uint8_t[n]); }

// the header's search on a table of 64-bit sums
static int pick(const std::vector<uint64_t>& size, int qmax, uint64_t budget) {
    if (size[qmax] <= budget) return qmax;
    int lo = 0, hi = qmax;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (size[mid] <= budget) lo = mid; else hi = mid; }
    return lo > 1 ? lo : 1;
}

static void one_sequence(int n, int w, int h, bool is444) {
    const size_t row = (size_t)w * 3 + 5, frame_stride = row * ((size_t)h - 1) + (size_t)w * 3 + 11, n_bgr = frame_stride * ((size_t)n - 1) + row * ((size_t)h - 1) + (size_t)w * 3;
    Bytes bgr = exact(n_bgr);
    for (size_t i = 0; i < n_bgr; ++i) bgr[i] = 0xA5;
    for (int k = 0; k < n; ++k)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < 3 * w; ++x) bgr[(size_t)k * frame_stride + (size_t)y * row + x] = k % 3 == 0 ? (uint8_t)next() : k % 3 == 1 ? (uint8_t)((next() & 1) * 255) : (uint8_t)140;
    const int fmt = is444 ? POPPY_FRAME_JPEG444 : POPPY_FRAME_JPEG;
    const size_t place = is444 ? (size_t)w * h * 3 : poppy_frame_bytes(POPPY_FRAME_I420, w, h), cap = poppy_frame_bytes(fmt, w, h);
    Bytes planes = exact(place * n);
    for (int k = 0; k < n; ++k)
        CHECK((is444 ? poppy_bgr_to_i444 : poppy_bgr_to_i420)(bgr.get() + (size_t)k * frame_stride, row, w, h, planes.get() + (size_t)k * place) == POPPY_OK, "the planes of frame %d", k);
    auto fixed = is444 ? poppy_i444_to_jpeg_frame : poppy_i420_to_jpeg_frame;
    auto of_planes = is444 ? poppy_i444_frames_to_jpeg_seq_budget_frames : poppy_i420_frames_to_jpeg_seq_budget_frames;
    auto of_bgr = is444 ? poppy_bgr_frames_to_jpeg444_seq_budget_frames : poppy_bgr_frames_to_jpeg_seq_budget_frames;
    std::vector<uint64_t> size(101, 0);
    std::vector<std::vector<Bytes>> frames(101);
    for (int q = 1; q <= 100; ++q)
        for (int k = 0; k < n; ++k) {
            frames[q].push_back(exact(cap));
            CHECK(fixed(planes.get() + (size_t)k * place, w, h, q, frames[q][k].get()) == POPPY_OK, "quality %d", q);
            size[q] += poppy_jpeg_frame_bytes(frames[q][k].get()) - 4;
        }
    Bytes got = exact(cap * n), got_bgr = exact(cap * n);
    const int qmaxes[] = {100, 50, 1};
    for (int qmax : qmaxes) {
        std::vector<uint64_t> budgets = {1, size[1] / 2 + 1, (uint64_t)cap * n, ((uint64_t)1 << 32) + size[50 < qmax ? 50 : qmax]};
        for (int q = 1; q <= 100; q += q < 6 ? 1 : 13) { budgets.push_back(size[q]); if (size[q] > 1) budgets.push_back(size[q] - 1); }
        for (uint64_t b : budgets) {
            const int want = pick(size, qmax, b);
            int used = -1;
            CHECK(of_planes(planes.get(), place, n, w, h, qmax, b, got.get(), &used) == POPPY_OK, "%d frames of %d x %d qmax %d budget %llu", n, w, h, qmax, (unsigned long long)b);
            CHECK(used == want, "%d frames of %d x %d qmax %d budget %llu: quality %d, the search on the sums gives %d", n, w, h, qmax, (unsigned long long)b, used, want);
            if (used < 1 || used > 100) continue;
            for (int k = 0; k < n; ++k) {
                const size_t total = poppy_jpeg_frame_bytes(got.get() + (size_t)k * cap);
                CHECK(total == poppy_jpeg_frame_bytes(frames[used][k].get()) && memcmp(got.get() + (size_t)k * cap, frames[used][k].get(), total) == 0,
                      "%d frames of %d x %d qmax %d budget %llu: frame %d is not its frame at quality %d", n, w, h, qmax, (unsigned long long)b, k, used);
                CHECK(poppy_jpeg_frame_quality(got.get() + (size_t)k * cap) == used, "the quality read back");
            }
            CHECK(size[used] <= b || (used == 1 && size[1] > b), "%d frames qmax %d budget %llu: %llu bytes at quality %d", n, qmax, (unsigned long long)b, (unsigned long long)size[used], used);
            int used_bgr = -1;
            CHECK(of_bgr(bgr.get(), row, frame_stride, n, w, h, qmax, b, got_bgr.get(), &used_bgr) == POPPY_OK && used_bgr == used, "the BGR statement's quality");
            for (int k = 0; k < n; ++k)
                CHECK(memcmp(got_bgr.get() + (size_t)k * cap, got.get() + (size_t)k * cap, poppy_jpeg_frame_bytes(got.get() + (size_t)k * cap)) == 0, "the BGR statement's frame %d", k);
        }
    }
}

int main() {
    const int sizes[][3] = {{1, 17, 9}, {2, 40, 24}, {5, 136, 24}, {3, 1, 1}, {2, 33, 1}};
    for (const auto& s : sizes)
        for (int is444 = 0; is444 < 2; ++is444) one_sequence(s[0], s[1], s[2], is444 != 0);
    // the refusals: nothing is read or written (the buffers are a byte long)
    Bytes one = exact(1);
    for (int is444 = 0; is444 < 2; ++is444) {
        auto f = is444 ? poppy_i444_frames_to_jpeg_seq_budget_frames : poppy_i420_frames_to_jpeg_seq_budget_frames;
        auto g = is444 ? poppy_bgr_frames_to_jpeg444_seq_budget_frames : poppy_bgr_frames_to_jpeg_seq_budget_frames;
        const size_t place = is444 ? 12 : 6;
        CHECK(f(nullptr, place, 2, 2, 2, 90, 9, one.get(), nullptr) == POPPY_E_ARG && f(one.get(), place, 2, 2, 2, 90, 9, nullptr, nullptr) == POPPY_E_ARG &&
              f(one.get(), place, 0, 2, 2, 90, 9, one.get(), nullptr) == POPPY_E_ARG && f(one.get(), place - 1, 2, 2, 2, 90, 9, one.get(), nullptr) == POPPY_E_ARG &&
              f(one.get(), place, 2, 0, 2, 90, 9, one.get(), nullptr) == POPPY_E_ARG && f(one.get(), place, 2, 2, 2, 0, 9, one.get(), nullptr) == POPPY_E_ARG &&
              f(one.get(), place, 2, 2, 2, 101, 9, one.get(), nullptr) == POPPY_E_ARG && f(one.get(), place, 2, 2, 2, 90, 0, one.get(), nullptr) == POPPY_E_ARG &&
              f(one.get(), (size_t)1 << 40, 2, 65536, 1, 90, 9, one.get(), nullptr) == POPPY_E_UNSUPPORTED, "the planes statement's refusals");
        CHECK(g(nullptr, 6, 12, 2, 2, 2, 90, 9, one.get(), nullptr) == POPPY_E_ARG && g(one.get(), 5, 12, 2, 2, 2, 90, 9, one.get(), nullptr) == POPPY_E_ARG &&
              g(one.get(), 6, 11, 2, 2, 2, 90, 9, one.get(), nullptr) == POPPY_E_ARG && g(one.get(), 6, 12, 0, 2, 2, 90, 9, one.get(), nullptr) == POPPY_E_ARG &&
              g(one.get(), 6, 12, 2, 2, 2, 90, 0, one.get(), nullptr) == POPPY_E_ARG && g(one.get(), 6, 12, 2, 2, 2, 101, 9, one.get(), nullptr) == POPPY_E_ARG &&
              g(one.get(), 3 * 65536, (size_t)1 << 40, 2, 65536, 1, 90, 9, one.get(), nullptr) == POPPY_E_UNSUPPORTED, "the BGR statement's refusals");
    }
    std::printf(g_failed ? "%d checks failed\n" : "jpeg sequence budget host check ok\n", g_failed);
    return g_failed ? 1 : 0;
}
