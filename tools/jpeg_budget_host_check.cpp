// jpeg_budget_host_check.cpp — the host statements of the JPEG byte budget (poppy_amd/csrc/frame_jpeg_budget.cpp over frame_jpeg.cpp's coder) alone, on the host,
// under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_budget_host_check.cpp poppy_amd/csrc/frame_jpeg_budget.cpp \
//       poppy_amd/csrc/frame_jpeg.cpp poppy_amd/csrc/frame_i444.cpp poppy_amd/csrc/frame_sink.cpp poppy_amd/csrc/frame_gif.cpp poppy_amd/csrc/frame_pal8.cpp \
//       poppy_amd/csrc/frame_png.cpp poppy_amd/csrc/frame_png_runs.cpp poppy_amd/csrc/frame_png_opt.cpp poppy_amd/csrc/frame_png_seq.cpp \
//       -o /tmp/jpeg_budget_asan && /tmp/jpeg_budget_asan
// (frame_sink.cpp defines poppy_bgr_to_i420 and poppy_frame_bytes and refers to the other formats' host statements; half a minute under the sanitizers.)
// Planes, BGR frames and size tables lie in heap buffers of EXACTLY their size and every frame in a buffer of exactly the format's capacity, so a byte read or
// written beside them is the sanitizer's to report.  Frames of noise, of saturated noise and flat ones at the sizes of tests/jpeg_budget_util.py, both samplings,
// every highest quality of that file; per frame the table of all 100 sizes from the fixed-quality statement, then per budget: the statement's quality is
// poppy_jpeg_budget_pick's on the table, its frame is the fixed-quality frame at that quality, poppy_jpeg_frame_quality reads the quality back, and the file fits
// unless the quality is 1.  The refusals last.  Returns 0 when every call returns what the rule promises.
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

static void one_frame(int w, int h, int kind, bool is444) {
    const size_t n_bgr = (size_t)w * h * 3;
    Bytes bgr = exact(n_bgr);
    for (size_t i = 0; i < n_bgr; ++i) bgr[i] = kind == 0 ? (uint8_t)next() : kind == 1 ? (uint8_t)((next() & 1) * 255) : (uint8_t)140;
    const int fmt = is444 ? POPPY_FRAME_JPEG444 : POPPY_FRAME_JPEG;
    const size_t n_planes = is444 ? n_bgr : poppy_frame_bytes(POPPY_FRAME_I420, w, h), cap = poppy_frame_bytes(fmt, w, h);
    Bytes planes = exact(n_planes);
    CHECK((is444 ? poppy_bgr_to_i444 : poppy_bgr_to_i420)(bgr.get(), (size_t)w * 3, w, h, planes.get()) == POPPY_OK, "the planes of %d x %d", w, h);
    auto fixed = is444 ? poppy_i444_to_jpeg_frame : poppy_i420_to_jpeg_frame;
    auto budgeted = is444 ? poppy_i444_to_jpeg_budget_frame : poppy_i420_to_jpeg_budget_frame;
    auto budgeted_bgr = is444 ? poppy_bgr_to_jpeg444_budget_frame : poppy_bgr_to_jpeg_budget_frame;
    std::unique_ptr<uint32_t[]> sizes(new uint32_t[101]);
    std::vector<Bytes> frames(101);
    sizes[0] = 0;
    for (int q = 1; q <= 100; ++q) {
        frames[q] = exact(cap);
        CHECK(fixed(planes.get(), w, h, q, frames[q].get()) == POPPY_OK, "quality %d", q);
        sizes[q] = (uint32_t)(poppy_jpeg_frame_bytes(frames[q].get()) - 4);
        CHECK(poppy_jpeg_frame_quality(frames[q].get()) == q, "quality %d read back as %d", q, poppy_jpeg_frame_quality(frames[q].get()));
    }
    Bytes got = exact(cap), got_bgr = exact(cap);
    const int qmaxes[] = {100, 90, 50, 2, 1};
    for (int qmax : qmaxes) {
        std::unique_ptr<uint32_t[]> table(new uint32_t[(size_t)qmax + 1]);      // exactly the entries the search may read
        memcpy(table.get(), sizes.get(), sizeof(uint32_t) * ((size_t)qmax + 1));
        std::vector<size_t> budgets = {1, sizes[1] / 2u + 1, (size_t)cap, 0xffffffffu};
        for (int q = 1; q <= 100; q += q < 10 ? 1 : 7) { budgets.push_back(sizes[q]); if (sizes[q] > 1) budgets.push_back(sizes[q] - 1); }
        for (size_t b : budgets) {
            const int want = poppy_jpeg_budget_pick(table.get(), qmax, b);
            int used = -1;
            CHECK(budgeted(planes.get(), w, h, qmax, b, got.get(), &used) == POPPY_OK, "%d x %d qmax %d budget %zu", w, h, qmax, b);
            CHECK(used == want && want >= 1 && want <= qmax, "%d x %d qmax %d budget %zu: quality %d, the search on the table gives %d", w, h, qmax, b, used, want);
            if (used < 1 || used > 100) continue;
            const size_t total = poppy_jpeg_frame_bytes(got.get());
            CHECK(total == (size_t)sizes[used] + 4 && memcmp(got.get(), frames[used].get(), total) == 0, "%d x %d qmax %d budget %zu: not the frame at quality %d", w, h, qmax, b, used);
            CHECK(sizes[used] <= b || (used == 1 && sizes[1] > b), "%d x %d qmax %d budget %zu: %u bytes at quality %d", w, h, qmax, b, sizes[used], used);
            CHECK(poppy_jpeg_frame_quality(got.get()) == used, "the quality read back");
            CHECK(budgeted_bgr(bgr.get(), (size_t)w * 3, w, h, qmax, b, got_bgr.get(), nullptr) == POPPY_OK && memcmp(got_bgr.get(), got.get(), total) == 0, "%d x %d qmax %d budget %zu: the BGR statement", w, h, qmax, b);
        }
    }
}

int main() {
    const int sizes[][2] = {{8, 8}, {17, 9}, {40, 24}, {24, 24}, {136, 24}, {1, 1}, {33, 1}};
    for (const auto& s : sizes)
        for (int kind = 0; kind < 3; ++kind)
            for (int is444 = 0; is444 < 2; ++is444) one_frame(s[0], s[1], kind, is444 != 0);
    // the refusals: nothing is read or written (the buffers are a byte long)
    Bytes one = exact(1);
    std::unique_ptr<uint32_t[]> t(new uint32_t[2]{0, 5});
    CHECK(poppy_jpeg_budget_pick(nullptr, 1, 5) == POPPY_E_ARG && poppy_jpeg_budget_pick(t.get(), 0, 5) == POPPY_E_ARG && poppy_jpeg_budget_pick(t.get(), 101, 5) == POPPY_E_ARG &&
          poppy_jpeg_budget_pick(t.get(), 1, 0) == POPPY_E_ARG && poppy_jpeg_budget_pick(t.get(), 1, 4) == 1 && poppy_jpeg_budget_pick(t.get(), 1, 5) == 1, "the search's refusals");
    for (int is444 = 0; is444 < 2; ++is444) {
        auto f = is444 ? poppy_i444_to_jpeg_budget_frame : poppy_i420_to_jpeg_budget_frame;
        auto g = is444 ? poppy_bgr_to_jpeg444_budget_frame : poppy_bgr_to_jpeg_budget_frame;
        CHECK(f(nullptr, 2, 2, 90, 9, one.get(), nullptr) == POPPY_E_ARG && f(one.get(), 2, 2, 90, 9, nullptr, nullptr) == POPPY_E_ARG && f(one.get(), 0, 2, 90, 9, one.get(), nullptr) == POPPY_E_ARG &&
              f(one.get(), 2, 2, 0, 9, one.get(), nullptr) == POPPY_E_ARG && f(one.get(), 2, 2, 101, 9, one.get(), nullptr) == POPPY_E_ARG && f(one.get(), 2, 2, 90, 0, one.get(), nullptr) == POPPY_E_ARG &&
              f(one.get(), 2, 2, 90, (size_t)1 << 32, one.get(), nullptr) == POPPY_E_ARG && f(one.get(), 65536, 1, 90, 9, one.get(), nullptr) == POPPY_E_UNSUPPORTED, "the planes statement's refusals");
        CHECK(g(nullptr, 6, 2, 2, 90, 9, one.get(), nullptr) == POPPY_E_ARG && g(one.get(), 5, 2, 2, 90, 9, one.get(), nullptr) == POPPY_E_ARG && g(one.get(), 6, 2, 2, 90, 0, one.get(), nullptr) == POPPY_E_ARG &&
              g(one.get(), 6, 2, 2, 90, (size_t)1 << 32, one.get(), nullptr) == POPPY_E_ARG && g(one.get(), 3 * 65536, 65536, 1, 90, 9, one.get(), nullptr) == POPPY_E_UNSUPPORTED, "the BGR statement's refusals");
    }
    Bytes four = exact(4);
    memset(four.get(), 0, 4);
    CHECK(poppy_jpeg_frame_quality(nullptr) == 0 && poppy_jpeg_frame_quality(four.get()) == 0, "a frame too short to hold a DQT is read no further than its length");
    std::printf(g_failed ? "%d checks failed\n" : "jpeg budget host check ok\n", g_failed);
    return g_failed ? 1 : 0;
}
