// denoise_host_check.cpp — the host statement of the non-local-means denoise (poppy_amd/csrc/denoise.cpp) alone, on the host, under the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/denoise_host_check.cpp \
//       poppy_amd/csrc/denoise.cpp -o /tmp/denoise_asan && /tmp/denoise_asan
// Every image lies in a heap buffer of EXACTLY its size (h rows of `stride` bytes, the last row cut after its pixels) and every table in a buffer of exactly
// n entries, so a byte written or read beside them is the sanitizer's to report.  The shapes are those of tests/denoise_util.py in kind: sides of 1, 2, 5,
// 13, 26 and 27 (every index folds, several times), a frame larger than both windows, rows with padding; flat 0 / 128 / 255, saturated noise and noise
// around 128; every window pair at its smallest and largest, strengths 0.5 .. 100; the refusals.  Checked on the way: flat images come back unchanged (the
// all-255 one passes 2^32 in the rounding sum), saturated noise comes back unchanged at hs 3, padding stays untouched, the table does not increase and ends
// at L.  Returns 0 when every call returns what the rule promises.
#include "../include/poppy_hip.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

static uint32_t g_state = 2463534242u;
static uint32_t next_u32() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }

static int g_calls = 0, g_failures = 0;

enum Content { kFlat0, kFlat128, kFlat255, kSaturated, kNoise };

// exactly (h - 1) * stride + 3 w bytes
static std::unique_ptr<uint8_t[]> image(int w, int h, size_t stride, Content c, uint8_t pad) {
    const size_t bytes = (size_t)(h - 1) * stride + (size_t)w * 3;
    std::unique_ptr<uint8_t[]> p(new uint8_t[bytes]);
    memset(p.get(), pad, bytes);
    for (int y = 0; y < h; ++y)
        for (int i = 0; i < w * 3; ++i) {
            uint8_t v = 0;
            switch (c) {
            case kFlat0: v = 0; break;
            case kFlat128: v = 128; break;
            case kFlat255: v = 255; break;
            case kSaturated: v = (next_u32() & 1u) ? 255 : 0; break;
            default: v = (uint8_t)(116 + next_u32() % 25u); break;
            }
            p[(size_t)y * stride + i] = v;
        }
    return p;
}

static void run(int w, int h, int src_pad, int dst_pad, Content c, float hs, int tw, int sw) {
    const size_t stride = (size_t)w * 3 + src_pad, dst_stride = (size_t)w * 3 + dst_pad;
    std::unique_ptr<uint8_t[]> src = image(w, h, stride, c, 0x5A), dst = image(w, h, dst_stride, kFlat0, 0xA5);
    memset(dst.get(), 0xA5, (size_t)(h - 1) * dst_stride + (size_t)w * 3);
    const int rc = poppy_bgr_denoise(src.get(), stride, w, h, hs, tw, sw, dst.get(), dst_stride);
    ++g_calls;
    bool ok = rc == POPPY_OK;
    const bool unchanged = c == kFlat0 || c == kFlat128 || c == kFlat255 || (c == kSaturated && hs <= 3.0f && tw == 7) || (w == 1 && h == 1);
    for (int y = 0; ok && y < h; ++y) {
        if (unchanged) ok = memcmp(dst.get() + (size_t)y * dst_stride, src.get() + (size_t)y * stride, (size_t)w * 3) == 0;
        for (int i = 0; ok && y + 1 < h && i < dst_pad; ++i) ok = dst[(size_t)y * dst_stride + (size_t)w * 3 + i] == 0xA5;
    }
    if (!ok) { fprintf(stderr, "%d x %d, pads %d / %d, content %d, (%g, %d, %d): rc %d\n", w, h, src_pad, dst_pad, (int)c, hs, tw, sw, rc); ++g_failures; }
}

static void table(float hs, int tw, int sw) {
    int n = 0, L = -1, shift = -1, n2 = 0; uint32_t fpm = 0;
    int rc = poppy_denoise_weights(hs, tw, sw, nullptr, 0, &n, &L, &fpm, &shift);
    ++g_calls;
    bool ok = rc == POPPY_OK && n > 0 && L >= 1 && L <= n && fpm > 0 && (1 << shift) >= tw * tw && (1 << shift) < 2 * tw * tw;
    if (ok) {
        std::unique_ptr<uint32_t[]> t(new uint32_t[n]);
        rc = poppy_denoise_weights(hs, tw, sw, t.get(), n, &n2, nullptr, nullptr, nullptr);
        ++g_calls;
        ok = rc == POPPY_OK && n2 == n && t[0] == fpm && t[L - 1] > 0;
        for (int a = 1; ok && a < n; ++a) ok = t[a] <= t[a - 1] && (a < L || t[a] == 0);
        if (ok && n > 1) {                                    // one entry short: refused, *n reported, nothing written
            std::unique_ptr<uint32_t[]> s(new uint32_t[n - 1]);
            n2 = 0;
            ok = poppy_denoise_weights(hs, tw, sw, s.get(), n - 1, &n2, nullptr, nullptr, nullptr) == POPPY_E_ARG && n2 == n;
            ++g_calls;
        }
    }
    if (!ok) { fprintf(stderr, "table (%g, %d, %d): rc %d, n %d, L %d\n", hs, tw, sw, rc, n, L); ++g_failures; }
}

static void refuse(const char* what, int want, int w, int h, size_t stride, size_t dst_stride, float hs, int tw, int sw, bool null_src, bool null_dst) {
    uint8_t src[8 * 6 * 3], dst[8 * 6 * 3];
    memset(src, 7, sizeof src); memset(dst, 0xA5, sizeof dst);
    const int rc = poppy_bgr_denoise(null_src ? nullptr : src, stride, w, h, hs, tw, sw, null_dst ? nullptr : dst, dst_stride);
    ++g_calls;
    bool ok = rc == want;
    for (size_t i = 0; ok && i < sizeof dst; ++i) ok = dst[i] == 0xA5;
    if (!ok) { fprintf(stderr, "%s: rc %d\n", what, rc); ++g_failures; }
}

int main() {
    const int windows[][2] = {{7, 21}, {5, 9}, {3, 3}, {3, 21}, {7, 3}};
    const int sizes[][2] = {{1, 1}, {1, 40}, {40, 1}, {2, 2}, {5, 3}, {13, 13}, {26, 27}, {27, 26}, {61, 33}};
    for (const auto& win : windows)
        for (const auto& s : sizes)
            for (Content c : {kFlat0, kFlat128, kFlat255, kSaturated, kNoise}) {
                if (win[0] != 7 && c != kNoise && c != kFlat255) continue;
                run(s[0], s[1], 0, 0, c, c == kSaturated ? 3.0f : 10.0f, win[0], win[1]);
            }
    for (float hs : {0.5f, 3.0f, 20.0f, 40.0f, 100.0f}) { run(33, 17, 0, 0, kNoise, hs, 7, 21); run(33, 17, 0, 0, kFlat255, hs, 7, 21); }
    run(37, 19, 5, 7, kNoise, 10.0f, 7, 21);
    run(37, 19, 1, 0, kNoise, 10.0f, 5, 9);
    run(1, 9, 0, 3, kNoise, 10.0f, 3, 3);
    for (const auto& win : windows)
        for (float hs : {0.5f, 3.0f, 10.0f, 20.0f, 40.0f, 100.0f}) table(hs, win[0], win[1]);
    const size_t S = 8 * 3;
    refuse("hs = 0", POPPY_E_ARG, 8, 6, S, S, 0.0f, 7, 21, false, false);
    refuse("hs < 0", POPPY_E_ARG, 8, 6, S, S, -1.0f, 7, 21, false, false);
    refuse("hs = NaN", POPPY_E_ARG, 8, 6, S, S, std::nanf(""), 7, 21, false, false);
    refuse("hs = inf", POPPY_E_ARG, 8, 6, S, S, INFINITY, 7, 21, false, false);
    refuse("tw even", POPPY_E_ARG, 8, 6, S, S, 10.0f, 6, 21, false, false);
    refuse("sw even", POPPY_E_ARG, 8, 6, S, S, 10.0f, 7, 20, false, false);
    refuse("tw = 0", POPPY_E_ARG, 8, 6, S, S, 10.0f, 0, 21, false, false);
    refuse("w = 0", POPPY_E_ARG, 0, 6, S, S, 10.0f, 7, 21, false, false);
    refuse("h < 0", POPPY_E_ARG, 8, -1, S, S, 10.0f, 7, 21, false, false);
    refuse("short stride", POPPY_E_ARG, 8, 6, S - 1, S, 10.0f, 7, 21, false, false);
    refuse("short dst stride", POPPY_E_ARG, 8, 6, S, S - 1, 10.0f, 7, 21, false, false);
    refuse("null src", POPPY_E_ARG, 8, 6, S, S, 10.0f, 7, 21, true, false);
    refuse("null dst", POPPY_E_ARG, 8, 6, S, S, 10.0f, 7, 21, false, true);
    refuse("tw = 1", POPPY_E_UNSUPPORTED, 8, 6, S, S, 10.0f, 1, 21, false, false);
    refuse("tw = 9", POPPY_E_UNSUPPORTED, 8, 6, S, S, 10.0f, 9, 21, false, false);
    refuse("sw = 1", POPPY_E_UNSUPPORTED, 8, 6, S, S, 10.0f, 7, 1, false, false);
    refuse("sw = 23", POPPY_E_UNSUPPORTED, 8, 6, S, S, 10.0f, 7, 23, false, false);
    printf("%d calls on buffers of exactly the images' and tables' sizes, %d failures\n", g_calls, g_failures);
    return g_failures ? 1 : 0;
}
