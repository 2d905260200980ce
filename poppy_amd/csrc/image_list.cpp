// image_list.cpp — poppy_hip_morph_list: the reference CLI's loop over an image list (src/poppy.cpp:266-328) in one call.  Pair k is
// (image k, image k + 1), where image k is what poppy::morph handed back as corrected2 for pair k - 1 (:326).  Pair 0 is set up with
// pair_begin, every later pair with pair_begin_next: the second image's filter chain of one pair is the first image's of the next, and
// it runs once.  Optional canvas: every image is padded on the device by blur_margin's rule (src/util.cpp:574-602) before its pair.  Optional denoise
// (poppy_hip_set_denoise, the CLI's --denoise at :172): every image goes through the non-local-means kernel first, at its own size.
#include "context.h"

namespace {

struct PairWriter {                       // poppy_write_cb -> poppy_write_pair_cb: the pair index and a running frame index
    poppy_write_pair_cb write; void* user; int pair; int frame;
};
void pair_writer_cb(void* u, const uint8_t* bgr, int w, int h, size_t stride) {
    PairWriter* p = static_cast<PairWriter*>(u);
    p->write(p->user, p->pair, p->frame++, bgr, w, h, stride);
}

struct ListImage {                        // one image as its pair reads it
    const uint8_t* p = nullptr; size_t stride = 0; int w = 0, h = 0; bool dev = false;
};

// the canvas scratch of the device-side blur_margin and the two padded images, kept by the context for UW x UH
int list_scratch(poppy_hip_ctx* c, int UW, int UH) {
    const size_t UB = (size_t)UW * UH * 3;
    if (c->bm_bytes >= UB && c->list_img_bytes >= UB + 16) return POPPY_OK;
    for (void* p : {(void*)c->bm_canvas, (void*)c->bm_tmp, (void*)c->list_img[0], (void*)c->list_img[1]}) if (p) (void)hipFree(p);
    c->bm_canvas = c->list_img[0] = c->list_img[1] = nullptr; c->bm_tmp = nullptr; c->bm_bytes = c->list_img_bytes = 0;
    HIPCHK(c, hipMalloc((void**)&c->bm_canvas, UB));
    HIPCHK(c, hipMalloc((void**)&c->bm_tmp, UB * 4));
    for (uint8_t*& p : c->list_img) HIPCHK(c, hipMalloc((void**)&p, UB + 16));
    c->bm_bytes = UB; c->list_img_bytes = UB + 16;
    if (!c->bm_taps) {
        const std::vector<int> taps = blur_margin_taps();
        HIPCHK(c, hipMalloc((void**)&c->bm_taps, taps.size() * 4));
        HIPCHK(c, hipMemcpy(c->bm_taps, taps.data(), taps.size() * 4, hipMemcpyHostToDevice));
    }
    return POPPY_OK;
}

// img -> out (UW x UH, tight rows, device): the bytes poppy_hip_blur_margin(img, UW, UH) returns, queued on the context's stream
int list_pad(poppy_hip_ctx* c, const ListImage& img, int UW, int UH, uint8_t* out) {
    int x0 = 0, y0 = 0;
    blur_margin_origin(img.w, img.h, UW, UH, &x0, &y0);
    HIPCHK(c, hipMemsetAsync(c->bm_canvas, 0, (size_t)UW * UH * 3, c->stream));
    HIPCHK(c, copy_rows_async(c->bm_canvas + ((size_t)y0 * UW + x0) * 3, (size_t)UW * 3, img.p, img.stride, (size_t)img.w * 3, img.h,
                              img.dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, blur_margin_strips(c->bm_canvas, out, c->bm_tmp, c->bm_taps, img.w, img.h, UW, UH, c->stream));
    return POPPY_OK;
}

// img -> out (its own size, tight rows, device): the bytes poppy_hip_denoise(img) returns, queued on the context's stream.  A host image goes through the
// context's staging image; a device image is read where it is and never written.
int list_denoise(poppy_hip_ctx* c, const ListImage& img, float hs, int tw, int sw, DeviceBuffer& out) {
    const size_t B = (size_t)img.w * img.h * 3;
    HIPCHK(c, out.reserve(B + 16, c->stream));
    const uint8_t* d_src = img.p; size_t stride = img.stride;
    if (!img.dev) {
        HIPCHK(c, c->denoise.stage.reserve(B, c->stream));
        HIPCHK(c, copy_rows_async(c->denoise.stage.p, (size_t)img.w * 3, img.p, img.stride, (size_t)img.w * 3, img.h, hipMemcpyHostToDevice, c->stream));
        d_src = c->denoise.stage.p; stride = (size_t)img.w * 3;
    }
    return denoise_queue(c, d_src, stride, out.p, img.w, img.h, hs, tw, sw);
}

}  // namespace

extern "C" {

int poppy_hip_morph_list(poppy_hip_ctx* c, int n, int UW, int UH, double phase, int inputs_on_device, poppy_image_source_cb source,
                         poppy_write_pair_cb write, void* user, double* morph_distances, int* pairs_done) {
    if (!c) return POPPY_E_ARG;
    if (pairs_done) *pairs_done = 0;
    if (!source || n < 2) return fail(c, POPPY_E_ARG, "morph_list: a source and at least two images");
    if (UW < 0 || UH < 0 || (UW == 0) != (UH == 0)) return fail(c, POPPY_E_ARG, "morph_list: canvas is 0 x 0 or both sides positive");
    if ((phase == 0 || phase == 1) && n > 2)     // poppy::morph returns before it sets corrected2 (src/poppy.hpp:54-70): nothing defines the next pair's image 1
        return fail(c, POPPY_E_UNSUPPORTED, "morph_list: phase 0 / 1 with more than two images");
    HIPCHK(c, hipSetDevice(c->device));
    const bool canvas = UW > 0;
    const int N = c->cfg.number_of_frames;
    int W = UW, H = UH;
    struct { float hs; int tw, sw; } const dn{c->denoise.hs, c->denoise.tw, c->denoise.sw};      // poppy_hip_set_denoise, as it stands when the call starts
    auto fetch = [&](int k, ListImage& img) -> int {            // image k from the source, checked against the list's geometry
        const uint8_t* p = nullptr; size_t stride = 0; int w = 0, h = 0;
        if (source(user, k, &p, &stride, &w, &h) != 0) return fail(c, POPPY_E_ARG, "morph_list: the image source failed");
        if (inputs_on_device) stride = (size_t)w * 3;
        if (!p || w <= 0 || h <= 0 || stride < (size_t)w * 3) return fail(c, POPPY_E_ARG, "morph_list: bad image from the source");
        if (canvas && (w > UW || h > UH)) return fail(c, POPPY_E_ARG, "morph_list: an image is larger than the canvas");
        if (canvas && poppy_blur_margin_rects(w, h, UW, UH, nullptr, nullptr) != POPPY_OK) return fail(c, POPPY_E_UNSUPPORTED, kBlurMarginOffCanvasMsg);
        if (canvas && !blur_margin_rows_fit(c, UH)) return fail(c, POPPY_E_UNSUPPORTED, kBlurMarginRowsMsg);
        if (!canvas) {
            if (k == 0) { W = w; H = h; }
            else if (w != W || h != H) return fail(c, POPPY_E_ARG, "morph_list: images of different sizes and no canvas (poppy::morph takes one size)");
        }
        img = ListImage{p, stride, w, h, inputs_on_device != 0};
        if (dn.hs != 0) {                                      // denoised at its own size, in front of the padding (src/poppy.cpp:172 before :239)
            const int rc = list_denoise(c, img, dn.hs, dn.tw, dn.sw, c->denoise.list_img[k & 1]); if (rc) return rc;
            img = ListImage{c->denoise.list_img[k & 1].p, (size_t)w * 3, w, h, true};
        }
        if (canvas) {                                         // padded into the context's image buffer k mod 2
            int rc = list_scratch(c, UW, UH); if (rc) return rc;
            rc = list_pad(c, img, UW, UH, c->list_img[k & 1]); if (rc) return rc;
            img = ListImage{c->list_img[k & 1], (size_t)UW * 3, UW, UH, true};
        }
        return POPPY_OK;
    };
    ListImage a, b;
    int rc = fetch(0, a); if (rc) return rc;
    rc = fetch(1, b); if (rc) return rc;
    if (phase == 0 || phase == 1) {                            // two images: poppy_hip_morph's short-circuit, before any feature work
        if (write) {                                           // (in the writer's format: converted on the device, or on the host for host images as poppy_hip_morph does)
            const ListImage& img = phase == 0 ? a : b;
            PairWriter pw{write, user, 0, 0};
            rc = img.dev ? write_device_image(c, img.p, W, H, N, pair_writer_cb, &pw) : write_host_image(c, img.p, img.stride, W, H, N, pair_writer_cb, &pw);
            if (rc) return rc;
        }
        if (pairs_done) *pairs_done = 1;
        return POPPY_OK;
    }
    for (int k = 0; k + 1 < n; ++k) {
        if (k > 0) { rc = fetch(k + 1, b); if (rc) return rc; }
        if (k == 0) rc = b.dev ? poppy_hip_pair_begin_device(c, a.p, b.p, W, H) : poppy_hip_pair_begin(c, a.p, a.stride, b.p, b.stride, W, H);
        else rc = b.dev ? poppy_hip_pair_begin_next_device(c, b.p, W, H) : poppy_hip_pair_begin_next(c, b.p, b.stride, W, H);
        if (rc) return rc;
        if (c->pts1_0.empty()) {                               // poppy_hip_morph's fallback: img2 * phase + img1 * (1 - phase), N times
            if (write) {
                const uint8_t* raw2 = c->c2_raw_valid ? c->c2_raw : c->c2;          // the image as it came in (auto-align may have replaced c2)
                launch_dissolve(raw2, c->c1, c->slots[0].out, (size_t)W * H * 3, (float)phase, (float)(1.0 - phase), c->stream);
                HIPCHK(c, hipGetLastError());
                PairWriter pw{write, user, k, 0};
                rc = write_device_image(c, c->slots[0].out, W, H, N, pair_writer_cb, &pw); if (rc) return rc;
                chain_touch(c);                                // as after poppy_hip_dissolve
                c->pair_ready = false;
            }
            return fail(c, POPPY_E_NOMATCH, "no point pairs: linear-blend fallback frames written (src/poppy.hpp:125-134)");
        }
        if (morph_distances) { rc = poppy_hip_pair_distance(c, &morph_distances[k]); if (rc) return rc; }
        PairWriter pw{write, user, k, 0};
        rc = poppy_hip_morph_frames(c, phase, write ? pair_writer_cb : nullptr, &pw); if (rc) return rc;
        if (pairs_done) *pairs_done = k + 1;
    }
    return POPPY_OK;
}

}  // extern "C"
