// ransac_host_check.cpp — the host statement of the RANSAC fundamental-matrix filter (poppy_amd/csrc/ransac_fundamental.cpp) alone, on the host, under the sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/ransac_host_check.cpp \
//       poppy_amd/csrc/ransac_fundamental.cpp -o /tmp/ransac_asan && /tmp/ransac_asan
// Every output lies in a heap buffer of EXACTLY its size (n mask bytes, 9 doubles, 2048 counts, 2048 x 9 model doubles) and the points in buffers of exactly
// n pairs, so a byte written or read beside them is the sanitizer's to report.  The scenes are those of tests/ransac_util.py in kind: two pinhole views of
// points at depth 4 .. 12 (the second camera turned 10 degrees about y and moved by (1, 0.1, 0.2)) with a quarter of unrelated pairs, at every size at which
// the sampler or a loop changes its shape and at both ends of the accepted range; identical pairs, a pure shift, collinear points, copies of one pair;
// coordinates scaled to +-1e6; distances 0, 3 and 1e9; the refusals.  Returns 0 when every call returns what the rule promises.
#include "../include/poppy_hip.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

static uint32_t g_state = 2463534242u;
static double uniform(double lo, double hi) { g_state = g_state * 1664525u + 1013904223u; return lo + (hi - lo) * ((g_state >> 8) / 16777216.0); }

struct Scene { std::unique_ptr<float[]> p1, p2; int n; };

static Scene two_view(int n, double scale) {
    Scene s{std::unique_ptr<float[]>(new float[2 * (size_t)n]), std::unique_ptr<float[]>(new float[2 * (size_t)n]), n};
    const double f = 800, cx = 640, cy = 480, ca = std::cos(10 * 3.14159265358979323846 / 180), sa = std::sin(10 * 3.14159265358979323846 / 180);
    for (int i = 0; i < n;) {
        double x1 = uniform(0, 1279), y1 = uniform(0, 959), x2, y2;
        if (i % 4 == 3) { x2 = uniform(0, 1279); y2 = uniform(0, 959); }
        else {
            const double z = uniform(4, 12), X = (x1 - cx) / f * z - 1.0, Y = (y1 - cy) / f * z - 0.1, Z = z - 0.2;
            const double xc = ca * X + sa * Z, zc = -sa * X + ca * Z;
            if (!(zc > 0)) continue;
            x2 = f * xc / zc + cx; y2 = f * Y / zc + cy;
            if (x2 < 0 || x2 > 1279 || y2 < 0 || y2 > 959) continue;
        }
        s.p1[2 * i] = (float)(x1 * scale); s.p1[2 * i + 1] = (float)(y1 * scale); s.p2[2 * i] = (float)(x2 * scale); s.p2[2 * i + 1] = (float)(y2 * scale);
        ++i;
    }
    return s;
}

static Scene degenerate(int kind) {
    const int n = 64;
    Scene s{std::unique_ptr<float[]>(new float[2 * n]), std::unique_ptr<float[]>(new float[2 * n]), n};
    for (int i = 0; i < n; ++i) {
        const double x = uniform(0, 1279), y = uniform(0, 959), t = uniform(0, 400);
        float* a = s.p1.get() + 2 * i; float* b = s.p2.get() + 2 * i;
        switch (kind) {
        case 0: a[0] = b[0] = (float)x; a[1] = b[1] = (float)y; break;
        case 1: a[0] = (float)x; a[1] = (float)y; b[0] = a[0] + 5.f; b[1] = a[1] + 3.f; break;
        case 2: a[0] = (float)(100 + t); a[1] = (float)(50 + 2 * t); b[0] = (float)(900 - 1.5 * t); b[1] = (float)(120 + t); break;
        default: a[0] = 321.5f; a[1] = 123.25f; b[0] = 328.5f; b[1] = 130.25f; break;
        }
    }
    return s;
}

static int g_calls = 0, g_failures = 0, g_models = 0;

static void run(const char* what, const Scene& s, double distance, bool want_no_model = false) {
    const int n = s.n;
    std::unique_ptr<uint8_t[]> mask(new uint8_t[n]);
    std::unique_ptr<double[]> f(new double[9]), models(new double[(size_t)POPPY_RANSAC_HYPOTHESES * 9]);
    std::unique_ptr<int[]> counts(new int[POPPY_RANSAC_HYPOTHESES]);
    int n_inliers = -7, best = -7;
    const bool lean = g_calls % 2 == 1;                    // every other call without the optional outputs
    const int rc = poppy_ransac_fundamental(s.p1.get(), s.p2.get(), n, distance, mask.get(), &n_inliers, f.get(), &best, lean ? nullptr : counts.get(), lean ? nullptr : models.get());
    ++g_calls;
    int kept = 0;
    bool ok = rc == POPPY_OK, zeros = true;
    for (int i = 0; ok && i < n; ++i) { ok = mask[i] <= 1; kept += mask[i]; }
    for (int k = 0; k < 9; ++k) { zeros = zeros && f[k] == 0.0; ok = ok && std::isfinite(f[k]); }
    ok = ok && kept == n_inliers && best >= -1 && best < POPPY_RANSAC_HYPOTHESES;
    if (best < 0) ok = ok && zeros && kept == n;
    else { ok = ok && !zeros && kept >= POPPY_RANSAC_MIN_POINTS && (lean || counts[best] == kept); ++g_models; }
    if (want_no_model) ok = ok && best == -1;
    if (!lean)
        for (int h = 0; ok && h < POPPY_RANSAC_HYPOTHESES; ++h) ok = counts[h] >= -1 && counts[h] <= n && (best < 0 || counts[h] < counts[best] || (counts[h] == counts[best] && h >= best));
    if (!ok) { fprintf(stderr, "%s, n %d, d %g: rc %d, best %d, %d inliers (mask %d)\n", what, n, distance, rc, best, n_inliers, kept); ++g_failures; }
}

static void refuse(const char* what, int n, double distance, bool null_mask) {
    Scene s = two_view(64, 1.0);
    uint8_t mask[64]; double f[9]; int n_inliers = -7, best = -7;
    const int rc = poppy_ransac_fundamental(s.p1.get(), s.p2.get(), n, distance, null_mask ? nullptr : mask, &n_inliers, f, &best, nullptr, nullptr);
    ++g_calls;
    if (rc != POPPY_E_ARG || n_inliers != -7 || best != -7) { fprintf(stderr, "%s: rc %d\n", what, rc); ++g_failures; }
}

int main() {
    for (int n : {8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 16385, POPPY_RANSAC_MAX_POINTS})
        for (double d : {3.0, 0.0, 1e9}) {
            if (n > 1025 && d != 3.0) continue;
            run("two views", two_view(n, 1.0), d);
        }
    run("two views, scaled to 1e6", two_view(256, 1e6 / 1280), 3.0);
    run("two views, negative and scaled", two_view(256, -1e6 / 1280), 3.0);
    const char* names[] = {"identical pairs", "pure shift", "collinear", "copies of one pair"};
    for (int kind = 0; kind < 4; ++kind)
        for (double d : {3.0, 0.0, 1e9}) run(names[kind], degenerate(kind), d, kind == 0 || kind == 3);
    refuse("n = 7", 7, 3.0, false);
    refuse("n = 65537", POPPY_RANSAC_MAX_POINTS + 1, 3.0, false);
    refuse("d < 0", 64, -1.0, false);
    refuse("d = NaN", 64, std::nan(""), false);
    refuse("d = inf", 64, INFINITY, false);
    refuse("null mask", 64, 3.0, true);
    printf("%d calls into buffers of exactly the outputs' sizes, %d with a model, %d failures\n", g_calls, g_models, g_failures);
    return g_failures ? 1 : 0;
}
