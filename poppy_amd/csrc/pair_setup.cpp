// pair_setup.cpp — the stage-by-stage entry points of the once-per-pair half of the C ABI (include/poppy_hip.h): ORB / descriptor / Hamming
// matching, the auto-align steps, the matcher, the stages of the pre-ORB filter chain (Extractor::foreground, medians, ORB input, gabor_filter),
// the host-side tables, blur_margin.  The set-up that runs them all from a raw pair is pair_begin.cpp; both share context.h.
#include "pair_begin.h"
#include "dft_exact.h"
#include "ransac_fundamental.h"
#include "gabor_doubt.h"

// blur_margin's two halves (src/util.cpp:574-602), shared by poppy_hip_blur_margin and poppy_hip_morph_list's device-side padding.
// taps: exp(-x^2 / 2 sigma^2) / sum in double, to 8 fractional bits with error diffusion, centre = 256 - rest (smooth.dispatch.cpp:224-258)
std::vector<int> blur_margin_taps() {
    const int n = kBlurMarginTaps; const double sigma = 6;
    std::vector<double> v(n); double sum = 0;
    for (int i = 0; i < n; ++i) { const double x = i - (n - 1) * 0.5; v[i] = std::exp(-(x * x) / (2 * sigma * sigma)); sum += v[i]; }
    std::vector<int> taps(n, 0);
    { double err = 0; int tot = 0;
      for (int i = 0; i < n / 2; ++i) { const double adj = v[i] / sum * 256 + err; const int v0 = (int)std::nearbyint(adj); err = adj - v0; taps[i] = taps[n - 1 - i] = v0; tot += v0; }
      taps[n / 2] = 256 - 2 * tot; }
    return taps;
}
// where a W x H image goes in the UW x UH canvas (its top-left pixel); the caller has checked the sizes
void blur_margin_origin(int W, int H, int UW, int UH, int* x0, int* y0) {
    int origin[2] = {0, 0};
    (void)poppy_blur_margin_rects(W, H, UW, UH, nullptr, origin);
    *x0 = origin[0]; *y0 = origin[1];
}
// the device's grid.y bound holds a strip's rows (launch_strip_blur: one grid row per strip row; the side strips are UH high)
bool blur_margin_rows_fit(const poppy_hip_ctx* c, int UH) { return UH <= c->max_grid_y; }
// canvas (the image already placed, zeros around it) -> out: the canvas, then the four margin strips blurred from it.
// Only for sizes poppy_blur_margin_rects admits: the entry points refuse the others before they come here, and so does this.
hipError_t blur_margin_strips(const uint8_t* canvas, uint8_t* out, uint32_t* tmp, const int* d_taps, int W, int H, int UW, int UH, hipStream_t s) {
    int rects[16];
    if (poppy_blur_margin_rects(W, H, UW, UH, rects, nullptr) != POPPY_OK) return hipErrorInvalidValue;
    hipError_t e = hipMemcpyAsync(out, canvas, (size_t)UW * UH * 3, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
    for (int k = 0; k < 4; ++k) {                      // left, right, top, bottom: later strips win; a strip of width or height 0 is skipped
        const int* r = rects + 4 * k;
        launch_strip_blur(canvas, out, UW, tmp, d_taps, kBlurMarginTaps, r[0], r[1], r[2], r[3], s);
    }
    return hipGetLastError();
}

extern "C" {

int poppy_hip_orb_detect(poppy_hip_ctx* c, const uint8_t* gray, size_t stride, int W, int H, int nfeatures, float* kps7, int max_kps, int* n_kps) {
    if (!c || !gray || !n_kps || W <= 0 || H <= 0 || stride < (size_t)W || nfeatures < 0) return POPPY_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    std::vector<OrbKeyPoint> kps;
    int n = c->orb.detect(gray, stride, W, H, nfeatures, c->stream, kps);
    if (n < 0) { c->err = "orb_detect: " + c->orb.err; return n == -2 ? POPPY_E_DEVICE : POPPY_E_ARG; }
    *n_kps = n;
    if (n > max_kps) return fail(c, POPPY_E_ARG, "max_kps too small");
    if (kps7) keypoint_rows7(kps, kps7);
    return POPPY_OK;
}

int poppy_hip_orb_describe(poppy_hip_ctx* c, const uint8_t* gray, size_t stride, int W, int H, const float* kps7, int n, uint8_t* desc) {
    if (!c || !gray || W <= 0 || H <= 0 || stride < (size_t)W || n < 0 || (n && (!kps7 || !desc))) return POPPY_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    int rc = c->orb.describe(gray, stride, W, H, kps7, n, c->stream, desc);
    if (rc < 0) { c->err = "orb_describe: " + c->orb.err; return rc == -2 ? POPPY_E_DEVICE : POPPY_E_ARG; }
    return POPPY_OK;
}

int poppy_hip_hamming_match(poppy_hip_ctx* c, const uint8_t* query, int nq, const uint8_t* train, int nt, int* out3, int* n_matches) {
    if (!c || nq < 0 || nt < 0 || !n_matches || (nq && !query) || (nt && !train) || (nq && nt && !out3)) return POPPY_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    int rc = c->orb.hamming(query, nq, train, nt, c->stream, out3);
    if (rc < 0) { c->err = "hamming_match: " + c->orb.err; return POPPY_E_DEVICE; }
    *n_matches = rc;
    return POPPY_OK;
}

int poppy_hip_hamming_knn2(poppy_hip_ctx* c, const uint8_t* query, int nq, const uint8_t* train, int nt, int* out4) {
    if (!c || nq < 0 || nt < 0 || (nq && !query) || (nt && !train) || (nq && !out4)) return POPPY_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    if (c->orb.hamming_knn2(query, nq, train, nt, c->stream, out4) < 0) { c->err = "hamming_knn2: " + c->orb.err; return POPPY_E_DEVICE; }
    return POPPY_OK;
}

int poppy_ratio_symmetry(const int* knn12, int n1, const int* knn21, int n2, float ratio, int* out3, int* n_out) {
    if (n1 < 0 || n2 < 0 || !n_out || (n1 && !knn12) || (n2 && !knn21)) return POPPY_E_ARG;
    std::vector<int> o;
    ratio_symmetry(knn12, n1, knn21, n2, ratio, o);
    *n_out = (int)o.size() / 3;
    if (out3 && !o.empty()) memcpy(out3, o.data(), o.size() * sizeof(int));
    return POPPY_OK;
}

// ---- auto-align ------------------------------------------------------------------------------------------------------
static int align_stage(poppy_hip_ctx* c, const uint8_t* img, size_t stride, int W, int H) {
    const size_t bytes = (size_t)W * H * 3;
    if (c->d_align_bytes < bytes) {
        if (c->d_align) (void)hipFree(c->d_align);
        c->d_align = nullptr; c->d_align_bytes = 0;
        HIPCHK(c, hipMalloc((void**)&c->d_align, bytes));
        c->d_align_bytes = bytes;
    }
    HIPCHK(c, copy_rows_async(c->d_align, (size_t)W * 3, img, stride, (size_t)W * 3, H, hipMemcpyHostToDevice, c->stream));
    return POPPY_OK;
}

int poppy_hip_warp_affine(poppy_hip_ctx* c, const uint8_t* src, size_t ss, int W, int H, const double* M, uint8_t* dst, size_t ds) {
    if (!c) return POPPY_E_ARG;
    if (!src || !dst || !M || W <= 0 || H <= 0 || ss < (size_t)W * 3 || ds < (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad warp_affine arguments");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = align_stage(c, src, ss, W, H); if (rc) return rc;
    uint8_t* d_out = nullptr; int* d_tab = nullptr;
    HIPCHK(c, hipMalloc((void**)&d_out, (size_t)W * H * 3));
    hipError_t e = hipMalloc((void**)&d_tab, (size_t)2 * (W + H) * sizeof(int));
    bool ok = e == hipSuccess && warp_affine_device(c->d_align, d_out, W, H, M, d_tab, c->stream);
    if (ok) ok = copy_rows_async(dst, ds, d_out, (size_t)W * 3, (size_t)W * 3, H, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                 hipStreamSynchronize(c->stream) == hipSuccess;
    (void)hipFree(d_out); if (d_tab) (void)hipFree(d_tab);
    return ok ? POPPY_OK : fail(c, POPPY_E_DEVICE, "warp_affine failed");
}

}  // extern "C"

// poppy_ransac_fundamental with the 2048 hypotheses on the GPU: the host normalises, the kernels fill counts and models on the set-up stream (own scratch: no
// resident buffer and no chain slot is touched), the host chooses, masks and refits (ransac_fundamental.cpp) — the same functions before and behind as the
// host statement runs, so the two differ in who computes counts and models, and in nothing else.
int ransac_filter(poppy_hip_ctx* c, const float* p1, const float* p2, int n, double distance, uint8_t* inliers, int* n_inliers, double* f3x3, int* best,
                  int* counts, double* models) {
    using namespace poppy_ransac;
    if (!p1 || !p2 || !inliers || !n_inliers || !f3x3 || !best) return fail(c, POPPY_E_ARG, "ransac: a required pointer is null");
    if (n < kMinPoints || n > kMaxPoints) return fail(c, POPPY_E_ARG, "ransac: takes 8 .. 65536 point pairs");
    if (!(distance >= 0.0) || !(distance <= 1.7976931348623157e308)) return fail(c, POPPY_E_ARG, "ransac: the distance must be finite and >= 0");
    std::vector<double> norm((size_t)n * 4), own_models;
    std::vector<int> own_counts;
    if (!counts) { own_counts.resize(kHypotheses); counts = own_counts.data(); }
    if (!models) { own_models.resize((size_t)kHypotheses * 9); models = own_models.data(); }
    Problem P;
    P.norm = norm.data();
    prepare(p1, p2, n, distance, P);
    if (P.normalised) {
        std::string err;
        const int rc = ransac_counts_device(c->ransac_scratch, c->stream, P, p1, p2, counts, models, err);
        if (rc) return fail(c, rc, err.c_str());
    } else models_and_counts(P, p1, p2, counts, models);        // no model: every count -1, every model zeros, nothing to launch
    finish(P, p1, p2, counts, models, inliers, n_inliers, f3x3, best);
    return POPPY_OK;
}

extern "C" {

static int align_host_entry(poppy_hip_ctx* c, int which, uint8_t* img, size_t stride, int W, int H, const float* p1, float* p2, int n, double* dist) {
    if (!c) return POPPY_E_ARG;
    if (!img || !p1 || !p2 || W <= 0 || H <= 0 || stride < (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad align arguments");
    if (n < 4 || n > kAlignMaxPoints) return fail(c, POPPY_E_ARG, kAlignCountError);
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    int rc = align_stage(c, img, stride, W, H); if (rc) return rc;
    std::vector<P2f> a(n), b(n);
    memcpy(a.data(), p1, (size_t)n * 8); memcpy(b.data(), p2, (size_t)n * 8);
    rc = which < 0 ? c->aligner.run(c->d_align, W, H, a, b, c->stream, dist) : c->aligner.step(which, c->d_align, W, H, a, b, c->stream, dist);
    if (rc) return fail(c, rc == -1 ? POPPY_E_ARG : POPPY_E_DEVICE, c->aligner.err.c_str());
    memcpy(p2, b.data(), (size_t)n * 8);
    HIPCHK(c, copy_rows_async(img, stride, c->d_align, (size_t)W * 3, (size_t)W * 3, H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return POPPY_OK;
}
int poppy_hip_auto_align(poppy_hip_ctx* c, uint8_t* img, size_t stride, int W, int H, const float* p1, float* p2, int n, double* dist) {
    return align_host_entry(c, -1, img, stride, W, H, p1, p2, n, dist);
}
int poppy_hip_align_step(poppy_hip_ctx* c, int which, uint8_t* img, size_t stride, int W, int H, const float* p1, float* p2, int n, double* dist) {
    if (which < 0 || which > 2) return c ? fail(c, POPPY_E_ARG, "align_step: which must be 0, 1 or 2") : POPPY_E_ARG;
    return align_host_entry(c, which, img, stride, W, H, p1, p2, n, dist);
}
int poppy_hip_align_scores(poppy_hip_ctx* c, const float* p1, const float* sets, int n, int n_cand, int W, int H, double* distances, float* totals,
                           int* n_pairs, float* inner_sums) {
    if (!c) return POPPY_E_ARG;
    if (!p1 || !sets || n_cand < 1 || W <= 0 || H <= 0) return fail(c, POPPY_E_ARG, "bad align arguments");
    if (n < 4 || n > kAlignMaxPoints) return fail(c, POPPY_E_ARG, kAlignCountError);
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    std::vector<P2f> a(n), b((size_t)n * n_cand);
    memcpy(a.data(), p1, (size_t)n * 8); memcpy(b.data(), sets, (size_t)n * n_cand * 8);
    std::vector<double> d;
    AutoAligner::ScoreParts parts;
    const int rc = c->aligner.scores(a, b, n_cand, W, H, c->stream, d, parts);
    if (rc) return fail(c, rc == -1 ? POPPY_E_ARG : POPPY_E_DEVICE, c->aligner.err.c_str());
    if (distances) memcpy(distances, d.data(), (size_t)n_cand * 8);
    if (totals) memcpy(totals, parts.total.data(), (size_t)n_cand * 4);
    if (n_pairs) memcpy(n_pairs, parts.n_pairs.data(), (size_t)n_cand * 4);
    if (inner_sums) memcpy(inner_sums, parts.inner.data(), (size_t)n_cand * 4);
    return POPPY_OK;
}
int poppy_procrustes(const float* x, const float* y, int n, float* rot4, float* se2, float* yprime) {
    if (!x || !y || n < 1) return POPPY_E_ARG;
    std::vector<P2f> a(n), b(n);
    memcpy(a.data(), x, (size_t)n * 8); memcpy(b.data(), y, (size_t)n * 8);
    ProcrustesFit f;
    procrustes_fit(a, b, f);
    if (rot4) memcpy(rot4, f.rotation, 16);
    if (se2) { se2[0] = f.scale; se2[1] = f.error; }
    if (yprime) memcpy(yprime, f.yprime.data(), (size_t)n * 8);
    return POPPY_OK;
}
int poppy_perspective_from4(const float* s4, const float* d4, double* m) {
    if (!s4 || !d4 || !m) return POPPY_E_ARG;
    perspective_from_4((const P2f*)s4, (const P2f*)d4, m);
    return POPPY_OK;
}

int poppy_match_points(const float* p1, const float* p2, int n, int W, int H, double tol, float* o1, float* o2, int* n_out, double* imd) {
    return match_points_with(nullptr, p1, p2, n, W, H, tol, o1, o2, n_out, imd);
}

int poppy_hip_foreground(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, uint8_t* out, const poppy_foreground_debug* dbg) {
    if (!c) return POPPY_E_ARG;
    if (!bgr || !out || W <= 0 || H <= 0 || stride < (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad image arguments");
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    ForegroundDebugOut d;
    if (dbg) { d.grey = dbg->grey; d.stages = dbg->stages; d.floats = dbg->floats; d.masked = dbg->masked; }
    const int rc = c->foreground.run(bgr, stride, W, H, c->stream, out, dbg ? &d : nullptr);
    if (rc) { c->err = "foreground: " + c->foreground.err; return rc == -1 ? POPPY_E_ARG : POPPY_E_DEVICE; }
    return POPPY_OK;
}

int poppy_hip_median_blur(poppy_hip_ctx* c, const uint8_t* src, int W, int H, int ksize, int form, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    const int rc = c->foreground.median(src, W, H, ksize, form, c->stream, dst);
    if (rc) { c->err = "median: " + c->foreground.err; return rc == -1 ? POPPY_E_ARG : POPPY_E_DEVICE; }
    return POPPY_OK;
}

int poppy_median_cols_geom(int W, int H, int* tiles_x, int* tiles_y, int* rows, int* tile_cols) {
    if (W <= 0 || H <= 0) return POPPY_E_ARG;
    const MedianColsGeom g = median_cols_geom(W, H);
    if (tiles_x) *tiles_x = g.tiles_x;
    if (tiles_y) *tiles_y = g.tiles_y;
    if (rows) *rows = g.rows;
    if (tile_cols) *tile_cols = g.cols;
    return POPPY_OK;
}
int poppy_median_cols_hint(const uint8_t* bgr, size_t stride, int W, int H) {
    if (!bgr || W <= 0 || H <= 0 || stride < (size_t)W * 3) return POPPY_E_ARG;
    return median_cols_hint_from_host(bgr, stride, W, H);
}
int poppy_hip_foreground_median_links(poppy_hip_ctx* c, int which, unsigned* cols_mask, int* decided_by) {
    if (!c || which < 0 || which > 1) return POPPY_E_ARG;
    const ForegroundFilter& fg = chain_fg(c, which);
    if (cols_mask) *cols_mask = fg.last_cols_mask;
    if (decided_by) *decided_by = fg.last_cols_decided_by;
    return POPPY_OK;
}

int poppy_hip_pair_corrected2(poppy_hip_ctx* c, uint8_t* dst, size_t ds) {
    if (!c || !dst) return POPPY_E_ARG;
    if (!c->pair_ready) return fail(c, POPPY_E_STATE, "no resident pair");
    if (ds < (size_t)c->W * 3) return fail(c, POPPY_E_ARG, "stride too small");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, copy_rows_async(dst, ds, c->c2, (size_t)c->W * 3, (size_t)c->W * 3, c->H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return POPPY_OK;
}

// intermediates of the last poppy_hip_pair_begin, for the tolerance tests: nfeatures, the two dft_detail2 values
int poppy_hip_ransac_fundamental(poppy_hip_ctx* c, const float* p1, const float* p2, int n, double distance, uint8_t* inliers, int* n_inliers, double* f3x3,
                                 int* best, int* counts, double* models) {
    if (!c) return POPPY_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return ransac_filter(c, p1, p2, n, distance, inliers, n_inliers, f3x3, best, counts, models);
}
int poppy_hip_pair_fundamental(poppy_hip_ctx* c, double* f3x3, int* n_matches, int* n_inliers, int* best) {
    if (!c) return POPPY_E_ARG;
    if (!c->pair_ready || !c->fundamental.valid) return fail(c, POPPY_E_STATE, "the resident pair was not set up by poppy_hip_pair_begin_descriptors_ransac");
    if (f3x3) memcpy(f3x3, c->fundamental.f, sizeof(c->fundamental.f));
    if (n_matches) *n_matches = c->fundamental.n_matches;
    if (n_inliers) *n_inliers = c->fundamental.n_inliers;
    if (best) *best = c->fundamental.best;
    return POPPY_OK;
}
int poppy_hip_pair_begin_info(poppy_hip_ctx* c, int* nfeatures, double* detail2) {
    if (!c) return POPPY_E_ARG;
    if (nfeatures) *nfeatures = c->last_nfeatures;
    if (detail2) { detail2[0] = c->last_detail[0]; detail2[1] = c->last_detail[1]; }
    return POPPY_OK;
}

// Extractor::keypoints' image chain for one goodFeatures image (host in / out): us = grey(unsharp), gb = Gabor mean, g = ORB input
int poppy_hip_orb_input(poppy_hip_ctx* c, const uint8_t* good_features, int W, int H, uint8_t* g, float* us, float* gb, double* detail) {
    if (!c || !good_features || W <= 0 || H <= 0) return POPPY_E_ARG;
    if (detail && !setup_size_ok(W, H)) return fail(c, POPPY_E_UNSUPPORTED, kSetupSizeMsg);
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    ForegroundFilter& fg = c->foreground;
    if (fg.prepare(W, H)) { c->err = "foreground: " + fg.err; return POPPY_E_DEVICE; }
    uint8_t* d_gf = fg.bgr_staging();                                   // any w*h device bytes will do as the staging area
    HIPCHK(c, hipMemcpyAsync(d_gf, good_features, (size_t)W * H, hipMemcpyHostToDevice, c->stream));
    if (detail && fg.detail(d_gf, W, H, c->stream, detail)) { c->err = "dft_detail2: " + fg.err; return POPPY_E_DEVICE; }
    const uint8_t* gi = fg.orb_input(d_gf, W, H, 0, c->stream, us, gb);
    if (!gi) { c->err = "orb_input: " + fg.err; return POPPY_E_DEVICE; }
    if (g) HIPCHK(c, hipMemcpyAsync(g, gi, (size_t)W * H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return POPPY_OK;
}

// 1: the Gabor banks as direct double-precision sums (kernels_prefilter2.hip), 0 (default): by tiled FFTs (kernels_gabor_fft.hip)
int poppy_hip_set_gabor_direct(poppy_hip_ctx* c, int on) {
    if (!c) return POPPY_E_ARG;
    c->foreground.gabor_direct = c->foreground_b.gabor_direct = on != 0;
    chain_touch(c);
    return POPPY_OK;
}

int poppy_hip_set_setup_chains(poppy_hip_ctx* c, int serial) {
    if (!c) return POPPY_E_ARG;
    c->setup_serial = serial != 0;
    return POPPY_OK;
}

int poppy_hip_gabor_doubt(unsigned long long out[3]) { return out && gabor_fft_doubt(out) ? POPPY_OK : POPPY_E_DEVICE; }

// gabor_filter(bgr / 255) with the default arguments (host in / out, f32x3)
int poppy_hip_gabor_field(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, float* out) {
    if (!c || !bgr || !out || W <= 0 || H <= 0 || stride < (size_t)W * 3) return POPPY_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    ForegroundFilter& fg = c->foreground;
    if (fg.prepare(W, H)) { c->err = "foreground: " + fg.err; return POPPY_E_DEVICE; }
    HIPCHK(c, copy_rows_async(fg.bgr_staging(), (size_t)W * 3, bgr, stride, (size_t)W * 3, H, hipMemcpyHostToDevice, c->stream));
    const float* gab = fg.gabor_field(fg.bgr_staging(), W, H, c->stream);
    if (!gab) { c->err = "gabor_field: " + fg.err; return POPPY_E_DEVICE; }
    HIPCHK(c, hipMemcpyAsync(out, gab, (size_t)W * H * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return POPPY_OK;
}

// blur_margin (src/util.cpp:574-602): what the reference's CLI does to every image before poppy::morph when the phase is not 0 / 1
// (src/poppy.cpp:233-240,293-308): centre it in the union canvas and blur the four margin strips (127x127, sigma 6, fixed point).
int poppy_hip_blur_margin(poppy_hip_ctx* c, const uint8_t* src, size_t stride, int W, int H, int UW, int UH, uint8_t* dst, size_t dst_stride) {
    if (!c) return POPPY_E_ARG;
    if (!src || !dst || W <= 0 || H <= 0 || UW < W || UH < H || stride < (size_t)W * 3 || dst_stride < (size_t)UW * 3) return fail(c, POPPY_E_ARG, "bad arguments");
    if (poppy_blur_margin_rects(W, H, UW, UH, nullptr, nullptr) != POPPY_OK) return fail(c, POPPY_E_UNSUPPORTED, kBlurMarginOffCanvasMsg);
    if (!blur_margin_rows_fit(c, UH)) return fail(c, POPPY_E_UNSUPPORTED, kBlurMarginRowsMsg);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t UB = (size_t)UW * UH * 3;
    uint8_t *canvas = nullptr, *out = nullptr; uint32_t* tmp = nullptr; int* d_taps = nullptr;
    auto cleanup = [&]() { for (void* p : {(void*)canvas, (void*)out, (void*)tmp, (void*)d_taps}) if (p) (void)hipFree(p); };
    const int n = kBlurMarginTaps;
    const std::vector<int> taps = blur_margin_taps();
    hipError_t e = hipMalloc((void**)&canvas, UB);
    if (e == hipSuccess) e = hipMalloc((void**)&out, UB);
    if (e == hipSuccess) e = hipMalloc((void**)&tmp, UB * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d_taps, n * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(d_taps, taps.data(), n * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(canvas, 0, UB, c->stream);
    int rx = 0, ry = 0;
    blur_margin_origin(W, H, UW, UH, &rx, &ry);
    if (e == hipSuccess) e = copy_rows_async(canvas + ((size_t)ry * UW + rx) * 3, (size_t)UW * 3, src, stride, (size_t)W * 3, H, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = blur_margin_strips(canvas, out, tmp, d_taps, W, H, UW, UH, c->stream);
    if (e != hipSuccess) { cleanup(); c->err = std::string("blur_margin: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    e = copy_rows_async(dst, dst_stride, out, (size_t)UW * 3, (size_t)UW * 3, UH, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    cleanup();
    if (e != hipSuccess) { c->err = std::string("blur_margin: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

// The one statement of blur_margin's geometry (src/util.cpp:580-595): rects = left, right, top, bottom as (x, y, width, height), origin = the
// image's top-left pixel in the canvas.  Either may be NULL.  Both are filled whenever the sizes are valid, also with POPPY_E_UNSUPPORTED.
int poppy_blur_margin_rects(int W, int H, int UW, int UH, int* rects, int* origin) {
    if (W <= 0 || H <= 0 || UW < W || UH < H) return POPPY_E_ARG;
    const double margin = ((double)W + (double)H) / 100.0;
    double dx = std::fabs((double)W - (double)UW) / 2.0, dy = std::fabs((double)H - (double)UH) / 2.0;
    if (origin) { origin[0] = (int)dx; origin[1] = (int)dy; }
    dx = (dx == 0 ? 1.3 : dx + margin);
    dy = (dy == 0 ? 1.3 : dy + margin);
    if (rects) {
        const int r[16] = {0, 0, (int)dx, UH,  (int)(UW - dx), 0, (int)dx, UH,  0, 0, UW, (int)dy,  0, (int)(UH - dy), UW, (int)dy};
        memcpy(rects, r, sizeof r);
    }
    return (int)dx > UW || (int)dy > UH ? POPPY_E_UNSUPPORTED : POPPY_OK;      // a strip leaves the canvas: the reference's Mat(Rect) throws
}
int poppy_blur_margin_taps(int* taps) {
    if (!taps) return POPPY_E_ARG;
    const std::vector<int> t = blur_margin_taps();
    memcpy(taps, t.data(), sizeof(int) * t.size());
    return POPPY_OK;
}
int poppy_hip_blur_margin_max_rows(poppy_hip_ctx* c, int* rows) {
    if (!c || !rows) return POPPY_E_ARG;
    *rows = c->max_grid_y;
    return POPPY_OK;
}

int poppy_dft_plan(int n, int* factors, int* n_factors, int* itab, float* wave) {
    if (n < 1 || !factors || !n_factors || !itab || !wave) return POPPY_E_ARG;
    DftPlanHost p;
    try { dft_make_plan(n, p); } catch (...) { return POPPY_E_UNSUPPORTED; }
    *n_factors = p.nf;
    memcpy(factors, p.factors, sizeof(int) * 34);
    memcpy(itab, p.itab.data(), sizeof(int) * (size_t)n);
    memcpy(wave, p.wave.data(), sizeof(float) * 2 * (size_t)n);
    return POPPY_OK;
}

// Host-side tables of the device code, for tests that run without a GPU.
// which = 31: Extractor::keypoints' bank (sigma 5, lambda 2), 13: gabor_filter's default bank (sigma 5, lambda 10).  bank: 16 * ks * ks floats
// (the kernels as getGaborKernel returns them); spectra: 8 * 4096 * 2 doubles = what kernels_gabor_fft.hip multiplies the patch spectrum with.
int poppy_gabor_tables(int which, float* bank, double* spectra) {
    if (which != 31 && which != 13) return POPPY_E_ARG;
    std::vector<float> b;
    gabor_bank(which, 5, which == 31 ? 2 : 10, 0.04, M_PI / 4, b);
    if (bank) memcpy(bank, b.data(), b.size() * 4);
    if (spectra) { const std::vector<double> t = gabor_fft_tables(b, which); memcpy(spectra, t.data(), t.size() * 8); }
    return POPPY_OK;
}
int poppy_gabor_rounding_in_doubt(double v, double band) { return rounding_in_doubt(v, band); }
double poppy_gabor_band_unit(void) { return gabor_band_unit(); }
// The tap table of the pyramid tail (kernels.h: PyrTailPlan) of a width x height frame: info[0..5] = first level of the tail, multi-pixel
// level steps, single-pixel reductions (-1: none), descriptors, LDS bytes, usable (0 / 1); desc (optional, room for info[3] * 4 words).
int poppy_pyr_tail_plan(int width, int height, int pyramid_levels, int tail_px, int* info, unsigned* desc) {
    if (width < 1 || height < 1 || pyramid_levels < 1 || pyramid_levels > 256 || !info) return POPPY_E_ARG;
    std::vector<PyrLevel> lv(pyramid_levels + 1);
    size_t o3 = 0, o1 = 0;
    int w = width, h = height;
    for (int i = 0; i <= pyramid_levels; ++i) { lv[i] = PyrLevel{w, h, o3, o1}; o3 += (size_t)w * h * 3; o1 += (size_t)w * h; w = (w + 1) / 2; h = (h + 1) / 2; }
    int first = pyramid_levels;
    for (int i = 1; i <= pyramid_levels; ++i) if ((size_t)lv[i].w * lv[i].h <= (size_t)tail_px) { first = i; break; }
    const PyrTailPlan p = build_pyr_tail_plan(lv.data(), first, pyramid_levels);
    info[0] = first; info[1] = p.args.n_wide; info[2] = p.args.nl; info[3] = p.args.n_desc; info[4] = (int)p.lds_bytes; info[5] = p.ok ? 1 : 0;
    if (desc && !p.desc.empty()) memcpy(desc, p.desc.data(), p.desc.size() * 4);
    return POPPY_OK;
}

int poppy_radial_gradient(int W, int H, float* out) {
    if (W <= 0 || H <= 0 || !out) return POPPY_E_ARG;
    std::vector<float> r;
    radial_gradient(W, H, r);
    memcpy(out, r.data(), r.size() * 4);
    return POPPY_OK;
}

int poppy_radial_mask(int W, int H, float* out) {
    if (W <= 0 || H <= 0 || !out) return POPPY_E_ARG;
    std::vector<float> r;
    radial_mask(W, H, r);
    memcpy(out, r.data(), r.size() * 4);
    return POPPY_OK;
}

}  // extern "C"
