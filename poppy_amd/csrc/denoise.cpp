// denoise.cpp — the host statement of the non-local-means denoise (include/poppy_hip.h: poppy_bgr_denoise) and the ONE place its weight table and
// constants are formed (poppy_denoise_weights): the GPU path uploads that table and never evaluates exp.  No GPU code and nothing of the context in
// here: tools/denoise_host_check.cpp builds this file alone, under the sanitizers.
#include "denoise.h"
#include "../../include/poppy_hip.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace poppy_denoise {

static_assert(kTileW == POPPY_DENOISE_TILE_W && kTileH == POPPY_DENOISE_TILE_H && kTableLds == POPPY_DENOISE_TABLE_LDS, "the header's constants");
static_assert(kMaxTemplate == POPPY_DENOISE_MAX_TEMPLATE && kMaxSearch == POPPY_DENOISE_MAX_SEARCH, "the header's constants");

int check_params(float hs, int tw, int sw, const char** why) {
    const char* msg = nullptr;
    int rc = POPPY_OK;
    if (!std::isfinite(hs) || !(hs > 0.0f)) { rc = POPPY_E_ARG; msg = "denoise: the strength is a finite float above 0"; }
    else if (tw <= 0 || sw <= 0 || tw % 2 == 0 || sw % 2 == 0) { rc = POPPY_E_ARG; msg = "denoise: the windows are odd"; }
    else if (tw < kMinWindow || tw > kMaxTemplate || sw < kMinWindow || sw > kMaxSearch) { rc = POPPY_E_UNSUPPORTED; msg = "denoise: template windows 3 .. 7 and search windows 3 .. 21 exist"; }
    if (why) *why = msg;
    return rc;
}

namespace {

struct Constants { uint32_t fpm; int shift, n; double mult; };

Constants constants(int tw, int sw) {
    Constants k;
    const uint64_t q = 0xFFFFFFFFull / ((uint64_t)sw * sw * 255);
    k.fpm = (uint32_t)(q < 0x7FFFFFFFull ? q : 0x7FFFFFFFull);
    k.shift = 0;
    while ((1 << k.shift) < tw * tw) ++k.shift;
    k.mult = (double)(1 << k.shift) / (double)(tw * tw);
    k.n = (int)((double)kMaxDist / k.mult) + 1;
    return k;
}

// t[0 .. n) and L, the index behind the last non-zero entry
int fill_table(float hs, const Constants& k, uint32_t* t) {
    const float den_f = (hs * hs) * 3.0f;                  // float, as the reference's expression evaluates; widened afterwards
    const double den = (double)den_f;
    const double floor_w = 0.001 * (double)k.fpm;
    int L = 0;
    for (int a = 0; a < k.n; ++a) {
        const double wd = std::exp(-((double)a * k.mult) / den);
        const double r = std::nearbyint((double)k.fpm * wd);          // round-half-even in the default rounding mode
        uint32_t v = (uint32_t)r;
        if ((double)v < floor_w) v = 0;
        t[a] = v;
        if (v) L = a + 1;
    }
    return L;
}

}  // namespace

}  // namespace poppy_denoise

using namespace poppy_denoise;

extern "C" {

int poppy_denoise_tile(int* tile_w, int* tile_h) {
    if (!tile_w || !tile_h) return POPPY_E_ARG;
    *tile_w = kTileW; *tile_h = kTileH;
    return POPPY_OK;
}

int poppy_denoise_table_bound(int* entries) {
    if (!entries) return POPPY_E_ARG;
    *entries = kTableLds;
    return POPPY_OK;
}

int poppy_denoise_weights(float hs, int tw, int sw, uint32_t* table, int cap, int* n, int* L, uint32_t* fpm, int* shift) {
    const int rc = check_params(hs, tw, sw, nullptr);
    if (rc) return rc;
    if (cap < 0 || (cap > 0 && !table)) return POPPY_E_ARG;
    const Constants k = constants(tw, sw);
    if (table && cap < k.n) { if (n) *n = k.n; return POPPY_E_ARG; }
    std::vector<uint32_t> own;
    uint32_t* t = table;
    if (!t) { own.resize((size_t)k.n); t = own.data(); }
    const int last = fill_table(hs, k, t);
    if (n) *n = k.n;
    if (L) *L = last;
    if (fpm) *fpm = k.fpm;
    if (shift) *shift = k.shift;
    return POPPY_OK;
}

int poppy_bgr_denoise(const uint8_t* src, size_t stride, int w, int h, float hs, int tw, int sw, uint8_t* dst, size_t dst_stride) {
    if (!src || !dst || w <= 0 || h <= 0 || stride < (size_t)w * 3 || dst_stride < (size_t)w * 3) return POPPY_E_ARG;
    const int rc = check_params(hs, tw, sw, nullptr);
    if (rc) return rc;
    const Constants k = constants(tw, sw);
    std::vector<uint32_t> t((size_t)k.n);
    const uint32_t L = (uint32_t)fill_table(hs, k, t.data());
    const int th = tw / 2, sh = sw / 2, b = th + sh;
    const int EW = w + 2 * b, EH = h + 2 * b;
    std::vector<uint8_t> e((size_t)EW * EH * 3);                       // the extended image
    for (int y = 0; y < EH; ++y) {
        const uint8_t* row = src + (size_t)fold101(y - b, h) * stride;
        for (int x = 0; x < EW; ++x) memcpy(&e[((size_t)y * EW + x) * 3], row + (size_t)fold101(x - b, w) * 3, 3);
    }
    // Per offset: the squared differences over the (w + 2 th) x (h + 2 th) pixels any template touches, and their integral; D of a pixel is four corners of it.
    const int SW = w + 2 * th, SH = h + 2 * th;
    std::vector<uint64_t> integral((size_t)(SW + 1) * (SH + 1), 0);
    std::vector<uint32_t> acc((size_t)w * h * 4, 0);                   // est[3], ws per pixel: unsigned 32 bits, as the rule says
    for (int dy = -sh; dy <= sh; ++dy)
        for (int dx = -sh; dx <= sh; ++dx) {
            for (int y = 0; y < SH; ++y) {
                const uint8_t* p = &e[((size_t)(y + sh) * EW + sh) * 3];
                const uint8_t* q = &e[((size_t)(y + sh + dy) * EW + sh + dx) * 3];
                const uint64_t* up = &integral[(size_t)y * (SW + 1)];
                uint64_t* out = &integral[(size_t)(y + 1) * (SW + 1)];
                uint64_t run = 0;
                for (int x = 0; x < SW; ++x) {
                    const int d0 = (int)p[3 * x] - (int)q[3 * x], d1 = (int)p[3 * x + 1] - (int)q[3 * x + 1], d2 = (int)p[3 * x + 2] - (int)q[3 * x + 2];
                    run += (uint64_t)(d0 * d0 + d1 * d1 + d2 * d2);
                    out[x + 1] = up[x + 1] + run;
                }
            }
            for (int y = 0; y < h; ++y) {
                const uint64_t* i0 = &integral[(size_t)y * (SW + 1)];
                const uint64_t* i1 = &integral[(size_t)(y + tw) * (SW + 1)];
                const uint8_t* q = &e[((size_t)(y + b + dy) * EW + b + dx) * 3];
                uint32_t* a4 = &acc[(size_t)y * w * 4];
                for (int x = 0; x < w; ++x) {
                    const uint64_t D = i1[x + tw] - i1[x] - i0[x + tw] + i0[x];
                    const uint32_t a = (uint32_t)(D >> k.shift);
                    const uint32_t wgt = a < L ? t[a] : 0u;
                    a4[4 * x] += wgt * q[3 * x]; a4[4 * x + 1] += wgt * q[3 * x + 1]; a4[4 * x + 2] += wgt * q[3 * x + 2];
                    a4[4 * x + 3] += wgt;
                }
            }
        }
    for (int y = 0; y < h; ++y) {
        uint8_t* out = dst + (size_t)y * dst_stride;
        const uint32_t* a4 = &acc[(size_t)y * w * 4];
        for (int x = 0; x < w; ++x) {
            const uint32_t ws = a4[4 * x + 3];                         // >= t[0] = fpm > 0: the centre offset has D = 0
            // est <= 255 ws < 2^32, but est + ws / 2 passes 2^32 on bright flat images at the widest search: the rounding sum is formed in 64 bits
            for (int c = 0; c < 3; ++c) out[3 * x + c] = (uint8_t)(((uint64_t)a4[4 * x + c] + ws / 2) / ws);
        }
    }
    return POPPY_OK;
}

}  // extern "C"
