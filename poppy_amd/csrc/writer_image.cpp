// writer_image.cpp — the frames that no slot renders (writer_image.h): a device or host image scaled and converted for the writer on the context's stream, and the
// stand-alone entry points that run one conversion kernel alone on buffers that live for the call.
#include "context.h"

int scale_into_scratch(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, const WriterGeom& g) {
    HIPCHK(c, c->scale_scratch.reserve(poppy_frame_bytes(POPPY_FRAME_BGR, g.w, g.h) + 16, c->stream));      // (the stream may still read the buffer that growth frees)
    launch_writer_scaling(g, d_bgr, c->scale_scratch.p, W, H, c->stream);
    HIPCHK(c, hipGetLastError());
    return POPPY_OK;
}

// what the coder of format `t` reads, in device memory (its raster form; PNG: the tight BGR frame) -> the coded frame in `host` (exactly `total` bytes), on the
// context's stream and waited for: the frames that no slot renders, and the stand-alone coding entry points.  d_tables: the JPEG coder's.  The buffers live for
// the call, at t's capacity; nothing of the call is in flight when they go.  budget (not empty: JPEG under a byte budget): the tables of all qualities and the budget's words.
static int coded_from_device(poppy_hip_ctx* c, const FormatTraits& t, const uint8_t* d_src, const void* d_tables, int W, int H, std::vector<uint8_t>& host, const JpegBudget& budget = JpegBudget()) {
    const size_t cap = capacity(t, (size_t)W, (size_t)H);
    CallBuffers held;
    uint8_t *work = nullptr, *frame = nullptr;
    hipError_t e = held.alloc(&work, coding_scratch_bytes(t, W, H));
    if (e == hipSuccess) e = held.alloc(&frame, cap + 16);
    if (e == hipSuccess) e = prepare_coding_scratch(t, work, W, H, c->stream);
    uint32_t total = 0;
    if (e == hipSuccess) {
        enqueue_coding(t, d_src, d_tables, work, frame, nullptr, W, H, c->stream, nullptr, nullptr, budget);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&total, frame, 4, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = e_sync;
    if (e == hipSuccess && !coded_length_ok(total, cap, t.least)) return fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds");
    if (e == hipSuccess) { host.resize(total); e = hipMemcpy(host.data(), frame, total, hipMemcpyDeviceToHost); }
    if (e != hipSuccess) { c->err = std::string(t.name) + " frame coding: " + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

int download_frame(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, const WriterGeom& g, std::vector<uint8_t>& host, size_t* stride, int n_copies) {
    const int fmt = c->frame_format;
    const FormatTraits& t = writer_traits(c, fmt);
    if (const char* why = format_refuses(fmt, g.w, g.h)) return fail(c, POPPY_E_UNSUPPORTED, why);
    if (g.scaled()) {                                              // scaled first, on the device; everything below is in the writer's geometry
        int rc = scale_into_scratch(c, d_bgr, W, H, g); if (rc) return rc;
        d_bgr = c->scale_scratch.p; W = g.w; H = g.h;
    }
    if (t.sequence) {                                              // the copies are the sequence: the host statement on the BGR frame
        std::vector<uint8_t> bgr((size_t)W * H * 3);
        HIPCHK(c, hipMemcpyAsync(bgr.data(), d_bgr, bgr.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        int rc = POPPY_OK;
        const uint8_t* frame = host_frame(c, bgr.data(), (size_t)W * 3, W, H, host, stride, &rc, n_copies);
        return frame ? POPPY_OK : rc;
    }
    *stride = writer_stride(fmt, W);
    const uint8_t* d_frame = d_bgr;
    JpegBudget budget;
    if (t.coder == kCoderJpeg) { int rc = ensure_jpeg_tables(c); if (rc) return rc; rc = context_jpeg_budget(c, t, &budget); if (rc) return rc; }
    if (t.raster != kRasterNone) {                                 // the raster step into the context's scratch: the slots' launches on other buffers
        if (t.raster == kRasterPal8) { int rc = alloc_zeroed_tables(c, &c->fmt_scratch_tables, kPal8TableBytes); if (rc) return rc; }
        HIPCHK(c, c->fmt_scratch.reserve(raster_bytes(t.raster, W, H) + 16, c->stream));
        SlotFormat scratch;
        scratch.i420 = scratch.i444 = scratch.pal8 = c->fmt_scratch.p; scratch.pal8_tables = c->fmt_scratch_tables;
        d_frame = enqueue_raster(t.raster, d_bgr, W, H, scratch, c->stream, nullptr, nullptr);
        HIPCHK(c, hipGetLastError());
    }
    if (t.coded()) return coded_from_device(c, t, d_frame, c->jpeg_tables, W, H, host, budget);      // the coder step, on buffers that live for the call
    host.resize(poppy_frame_bytes(fmt, W, H));
    HIPCHK(c, hipMemcpyAsync(host.data(), d_frame, host.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return POPPY_OK;
}

const uint8_t* host_frame(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, std::vector<uint8_t>& tmp, size_t* out_stride, int* status, int n_copies) {
    const int fmt = c->frame_format;
    const FormatTraits& t = writer_traits(c, fmt);
    *out_stride = stride;
    *status = POPPY_OK;
    if (t.raster == kRasterNone && !t.coded()) return bgr;
    if (const char* why = format_refuses(fmt, W, H)) { *status = fail(c, POPPY_E_UNSUPPORTED, why); return nullptr; }
    tmp.resize(poppy_frame_bytes(fmt, W, H));
    std::vector<uint8_t> pal8(t.sequence && t.coder == kCoderGif ? raster_bytes(kRasterPal8, W, H) : 0);      // (GIF_SEQ: PAL8_SEQ's frame, then the host coder)
    int rc = POPPY_OK;                                             // the host statement of the record's steps
    if (t.sequence && t.coder == kCoderJpeg && !t.frame_tables) rc = jpeg_seq_budget_of_copies(bgr, stride, std::max(1, n_copies), W, H, c->jpeg_quality, c->jpeg_seq_budget, fmt, tmp.data());
    else if (t.sequence && t.coder == kCoderJpeg) rc = jpeg_seq_of_copies(bgr, stride, std::max(1, n_copies), W, H, c->jpeg_quality, fmt, tmp.data());
    else if (t.sequence && t.coder == kCoderPng) rc = png_seq_of_copies(bgr, stride, std::max(1, n_copies), W, H, tmp.data());
    else if (t.sequence) rc = pal8_seq_of_copies(bgr, stride, std::max(1, n_copies), W, H, pal8.empty() ? tmp.data() : pal8.data());
    else if (t.coder == kCoderGif) rc = poppy_bgr_to_gif_frame(bgr, stride, W, H, tmp.data());
    else if (t.coder == kCoderJpeg && t.frame_tables) rc = (t.sampling() == jpeg::k444 ? poppy_bgr_to_jpeg444_opt_frame : poppy_bgr_to_jpeg_opt_frame)(bgr, stride, W, H, c->jpeg_quality, tmp.data());
    else if (t.coder == kCoderJpeg && c->jpeg_budget) rc = (t.sampling() == jpeg::k444 ? poppy_bgr_to_jpeg444_budget_frame : poppy_bgr_to_jpeg_budget_frame)(bgr, stride, W, H, c->jpeg_quality, c->jpeg_budget, tmp.data(), nullptr);
    else if (t.coder == kCoderJpeg) rc = (t.sampling() == jpeg::k444 ? poppy_bgr_to_jpeg444_frame : poppy_bgr_to_jpeg_frame)(bgr, stride, W, H, c->jpeg_quality, tmp.data());
    else if (t.coder == kCoderPng) rc = (t.variant == png::kRunsOwn ? poppy_bgr_to_png_opt_frame : t.runs() ? poppy_bgr_to_png_runs_frame : poppy_bgr_to_png_frame)(bgr, stride, W, H, tmp.data());
    else rc = (t.raster == kRasterPal8 ? poppy_bgr_to_pal8 : poppy_bgr_to_i420)(bgr, stride, W, H, tmp.data());
    if (rc == POPPY_OK && !pal8.empty()) rc = poppy_pal8_to_gif_frame(pal8.data(), W, H, tmp.data());
    if (rc) { *status = fail(c, rc, "the frame format refuses this frame"); return nullptr; }
    *out_stride = writer_stride(fmt, W);
    return tmp.data();
}

int write_device_image(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, int n_copies, poppy_write_cb write, void* user) {
    if (const char* why = writer_refuses(c, c->frame_format, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    const WriterGeom g = context_geom(c, W, H);
    std::vector<uint8_t> host; size_t stride = 0;
    int rc = download_frame(c, d_bgr, W, H, g, host, &stride, n_copies); if (rc) return rc;
    for (int j = 0; j < n_copies; ++j) write(user, host.data(), g.w, g.h, stride);
    return POPPY_OK;
}
int write_host_image(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, int n_copies, poppy_write_cb write, void* user) {
    if (const char* why = writer_refuses(c, c->frame_format, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    const WriterGeom g = context_geom(c, W, H);
    std::vector<uint8_t> small, tmp; int rc = POPPY_OK;
    if (g.scaled()) {                                              // the host statement, then the format's as for any host image
        small.resize(poppy_frame_bytes(POPPY_FRAME_BGR, g.w, g.h));
        rc = g.kind == kScaleSize ? poppy_bgr_resize_area(bgr, stride, W, H, g.w, g.h, small.data(), (size_t)g.w * 3)
                                  : poppy_bgr_downscale(bgr, stride, W, H, g.scale, small.data(), (size_t)g.w * 3);
        if (rc) return fail(c, rc, "the frame could not be scaled");
        bgr = small.data(); stride = (size_t)g.w * 3;
    }
    const uint8_t* frame = host_frame(c, bgr, stride, g.w, g.h, tmp, &stride, &rc, n_copies);
    if (!frame) return rc;
    for (int j = 0; j < n_copies; ++j) write(user, frame, g.w, g.h, stride);
    return POPPY_OK;
}

extern "C" {

int poppy_hip_bgr_resize_area_form(int W, int H, int ow, int oh) {
    if (!size_admits(W, H, ow, oh)) return POPPY_E_ARG;
    return bgr_resize_area_form(W, H, ow, oh);
}

// a host BGR frame up on the context's stream, tight, into a buffer that lives for the call (`held`).  Its place behind a 256-byte boundary is the row pad's low
// bits (include/poppy_hip.h): *d_src is that many bytes into the allocation.
static hipError_t upload_host_bgr(poppy_hip_ctx* c, CallBuffers& held, const uint8_t* bgr, size_t stride, int W, int H, uint8_t** d_src) {
    const size_t row = (size_t)W * 3, shift = (stride - row) % 16;
    hipError_t e = held.alloc(d_src, row * H + shift + 16);
    if (e != hipSuccess) return e;
    *d_src += shift;
    return copy_rows_async(*d_src, row, bgr, stride, row, (size_t)H, hipMemcpyHostToDevice, c->stream);
}

// the body of the two stand-alone scaling entries: a host frame W x H up, scaled to g on the device, down again, on buffers that live for the call
static int scale_host_frame(poppy_hip_ctx* c, const char* what, const uint8_t* bgr, size_t stride, int W, int H, const WriterGeom& g, uint8_t* dst, size_t dst_stride) {
    HIPCHK(c, hipSetDevice(c->device));
    const size_t out_row = (size_t)g.w * 3;
    CallBuffers held;
    uint8_t *d_src = nullptr, *d_dst = nullptr;
    hipError_t e = held.alloc(&d_dst, out_row * g.h + 16);
    if (e == hipSuccess) e = upload_host_bgr(c, held, bgr, stride, W, H, &d_src);
    if (e == hipSuccess) { launch_writer_scaling(g, d_src, d_dst, W, H, c->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = copy_rows_async(dst, dst_stride, d_dst, out_row, out_row, (size_t)g.h, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);     // nothing of the call is in flight when its buffers go (`held`, at the return)
    if (e == hipSuccess) e = e_sync;
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string(what) + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

int poppy_hip_bgr_resize_area(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, int ow, int oh, uint8_t* dst, size_t dst_stride) {
    if (!c) return POPPY_E_ARG;
    if (!bgr || !dst || !size_admits(W, H, ow, oh) || stride < (size_t)W * 3 || dst_stride < (size_t)ow * 3) return fail(c, POPPY_E_ARG, "bad arguments");
    return scale_host_frame(c, "BGR resize: ", bgr, stride, W, H, sized_geom(ow, oh), dst, dst_stride);
}

int poppy_hip_bgr_downscale(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, int factor, uint8_t* dst, size_t dst_stride) {
    if (!c) return POPPY_E_ARG;
    int ow = 0, oh = 0;
    if (!bgr || !dst || poppy_frame_scaled_size(W, H, factor, &ow, &oh) != POPPY_OK || stride < (size_t)W * 3 || dst_stride < (size_t)ow * 3)
        return fail(c, POPPY_E_ARG, "bad arguments");
    return scale_host_frame(c, "BGR downscale: ", bgr, stride, W, H, WriterGeom{ow, oh, factor, kScaleFactor}, dst, dst_stride);
}

int poppy_hip_pal8_to_gif_frame(poppy_hip_ctx* c, const uint8_t* pal8, int W, int H, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    if (!pal8 || !dst || W <= 0 || H <= 0) return fail(c, POPPY_E_ARG, "bad arguments");
    if (const char* why = format_refuses(POPPY_FRAME_GIF, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = poppy_frame_bytes(POPPY_FRAME_PAL8, W, H);
    CallBuffers held;                                              // (coded_from_device waits for the stream before it returns)
    uint8_t* d_pal8 = nullptr;
    HIPCHK(c, held.alloc(&d_pal8, bytes + 16));
    if (hipMemcpy(d_pal8, pal8, bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(c, POPPY_E_DEVICE, "upload of the PAL8 frame failed");
    std::vector<uint8_t> host;
    const int rc = coded_from_device(c, *format_traits(POPPY_FRAME_GIF), d_pal8, nullptr, W, H, host);
    if (rc == POPPY_OK) memcpy(dst, host.data(), host.size());
    return rc;
}

// the body of poppy_hip_i420_to_jpeg_frame, poppy_hip_i444_to_jpeg_frame and their OPT forms: the planes of format `fmt`'s sampling up, its kernels, `total` bytes down
static int jpeg_code_host_planes(poppy_hip_ctx* c, int fmt, const uint8_t* i420, int W, int H, int quality, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    if (!i420 || !dst || W <= 0 || H <= 0 || quality < 1 || quality > 100) return fail(c, POPPY_E_ARG, "bad arguments");
    if (const char* why = format_refuses(fmt, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    HIPCHK(c, hipSetDevice(c->device));
    const FormatTraits& traits = *format_traits(fmt);
    const size_t bytes = raster_bytes(traits.raster, W, H);
    jpeg::QualityTables t;
    jpeg::fill_quality_tables(quality, &t);
    CallBuffers held;                                              // (coded_from_device waits for the stream before it returns)
    uint8_t *d_i420 = nullptr, *d_tables = nullptr;
    HIPCHK(c, held.alloc(&d_i420, bytes + 16));
    HIPCHK(c, held.alloc(&d_tables, kJpegTableBytes));
    if (hipMemcpy(d_i420, i420, bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_tables, &t, sizeof t, hipMemcpyHostToDevice) != hipSuccess)
        return fail(c, POPPY_E_DEVICE, "upload of the planes failed");
    std::vector<uint8_t> host;
    const int rc = coded_from_device(c, traits, d_i420, d_tables, W, H, host);
    if (rc == POPPY_OK) memcpy(dst, host.data(), host.size());
    return rc;
}

int poppy_hip_i420_to_jpeg_frame(poppy_hip_ctx* c, const uint8_t* i420, int W, int H, int quality, uint8_t* dst) {
    return jpeg_code_host_planes(c, POPPY_FRAME_JPEG, i420, W, H, quality, dst);
}

// the body of poppy_hip_i420_to_jpeg_budget_frame and its I444 twin: the planes and the call's own budget words up, the search and the two coding kernels on the
// context's tables of all qualities, `total` bytes down; the quality is read back from the frame's DQT
static int jpeg_budget_code_host_planes(poppy_hip_ctx* c, int fmt, const uint8_t* planes, int W, int H, int quality_max, size_t budget, uint8_t* dst, int* quality_used) {
    if (!c) return POPPY_E_ARG;
    if (!planes || !dst || W <= 0 || H <= 0 || quality_max < 1 || quality_max > 100 || budget == 0 || budget > 0xffffffffull) return fail(c, POPPY_E_ARG, "bad arguments");
    if (const char* why = format_refuses(fmt, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    HIPCHK(c, hipSetDevice(c->device));
    const FormatTraits& traits = *format_traits(fmt);
    const size_t bytes = raster_bytes(traits.raster, W, H);
    { int rc = ensure_jpeg_budget_tables(c); if (rc) return rc; }      // (the context's tables of all qualities; its own budget is neither read nor touched)
    JpegBudget of_call;
    of_call.tables = c->jpeg_budget_tables;
    const JpegBudgetParams p{(uint32_t)budget, (uint32_t)quality_max};
    CallBuffers held;                                              // (coded_from_device waits for the stream before it returns)
    uint8_t *d_planes = nullptr, *d_params = nullptr;
    HIPCHK(c, held.alloc(&d_planes, bytes + 16));
    HIPCHK(c, held.alloc(&d_params, sizeof p));
    if (hipMemcpy(d_planes, planes, bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_params, &p, sizeof p, hipMemcpyHostToDevice) != hipSuccess)
        return fail(c, POPPY_E_DEVICE, "upload of the planes failed");
    of_call.params = d_params;
    std::vector<uint8_t> host;
    const int rc = coded_from_device(c, traits, d_planes, nullptr, W, H, host, of_call);
    if (rc != POPPY_OK) return rc;
    memcpy(dst, host.data(), host.size());
    if (quality_used) *quality_used = poppy_jpeg_frame_quality(dst);
    return POPPY_OK;
}
int poppy_hip_i420_to_jpeg_budget_frame(poppy_hip_ctx* c, const uint8_t* i420, int W, int H, int quality_max, size_t budget, uint8_t* dst, int* quality_used) {
    return jpeg_budget_code_host_planes(c, POPPY_FRAME_JPEG, i420, W, H, quality_max, budget, dst, quality_used);
}
int poppy_hip_i444_to_jpeg_budget_frame(poppy_hip_ctx* c, const uint8_t* i444, int W, int H, int quality_max, size_t budget, uint8_t* dst, int* quality_used) {
    return jpeg_budget_code_host_planes(c, POPPY_FRAME_JPEG444, i444, W, H, quality_max, budget, dst, quality_used);
}

int poppy_hip_i444_to_jpeg_frame(poppy_hip_ctx* c, const uint8_t* i444, int W, int H, int quality, uint8_t* dst) {
    return jpeg_code_host_planes(c, POPPY_FRAME_JPEG444, i444, W, H, quality, dst);
}

int poppy_hip_i420_to_jpeg_opt_frame(poppy_hip_ctx* c, const uint8_t* i420, int W, int H, int quality, uint8_t* dst) {
    return jpeg_code_host_planes(c, POPPY_FRAME_JPEG_OPT, i420, W, H, quality, dst);
}

int poppy_hip_i444_to_jpeg_opt_frame(poppy_hip_ctx* c, const uint8_t* i444, int W, int H, int quality, uint8_t* dst) {
    return jpeg_code_host_planes(c, POPPY_FRAME_JPEG444_OPT, i444, W, H, quality, dst);
}

// the table-build kernel alone on one table's counts (they stand as AC table 0 of a frame's count tables, the other three tables empty): what
// poppy_jpeg_optimal_table gives, with its refusals
int poppy_hip_jpeg_optimal_table(poppy_hip_ctx* c, const uint32_t* counts, uint8_t* bits, uint8_t* vals, int* n_vals) {
    if (!c) return POPPY_E_ARG;
    if (!counts || !bits || !vals || !n_vals) return fail(c, POPPY_E_ARG, "bad arguments");
    uint64_t sum = 0;
    for (int i = 0; i < 256; ++i) sum += counts[i];
    if (sum == 0 || sum >= 0xffffffffull) return fail(c, POPPY_E_ARG, "the counts are all zero, or their sum is 2^32 - 1 or more");
    HIPCHK(c, hipSetDevice(c->device));
    jpeg::SymbolCounts frame_counts{};
    memcpy(frame_counts.ac[0], counts, sizeof frame_counts.ac[0]);
    jpeg::OptTables built;
    CallBuffers held;
    uint8_t *d_counts = nullptr, *d_built = nullptr;
    HIPCHK(c, held.alloc(&d_counts, sizeof frame_counts));
    HIPCHK(c, held.alloc(&d_built, sizeof built));
    hipError_t e = hipMemcpyAsync(d_counts, &frame_counts, sizeof frame_counts, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch_jpeg_table_build((uint32_t*)d_counts, d_built, c->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(&built, d_built, sizeof built, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);     // nothing of the call is in flight when its buffers go (`held`, at the return)
    if (e == hipSuccess) e = e_sync;
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("JPEG table build: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    if (built.n[1] < 1 || built.n[1] > 256) return fail(c, POPPY_E_DEVICE, "the built table's size is outside its bounds");
    memcpy(bits, built.dht[1] + 1, 16);
    memcpy(vals, built.dht[1] + 17, built.n[1]);
    *n_vals = (int)built.n[1];
    return POPPY_OK;
}

// a host frame up (upload_host_bgr), the six PNG kernels, `total` bytes down, on buffers that live for the call
static int png_code_host_frame(poppy_hip_ctx* c, int fmt, const uint8_t* bgr, size_t stride, int W, int H, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    if (!bgr || !dst || W <= 0 || H <= 0 || stride < (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad arguments");
    if (const char* why = format_refuses(fmt, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    HIPCHK(c, hipSetDevice(c->device));
    CallBuffers held;                                              // (coded_from_device waits for the stream before it returns)
    uint8_t* d_src = nullptr;
    if (upload_host_bgr(c, held, bgr, stride, W, H, &d_src) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return fail(c, POPPY_E_DEVICE, "upload of the BGR frame failed");
    }
    std::vector<uint8_t> host;
    const int rc = coded_from_device(c, *format_traits(fmt), d_src, nullptr, W, H, host);
    if (rc == POPPY_OK) memcpy(dst, host.data(), host.size());
    return rc;
}
int poppy_hip_bgr_to_png_frame(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, uint8_t* dst) {
    return png_code_host_frame(c, POPPY_FRAME_PNG, bgr, stride, W, H, dst);
}
int poppy_hip_bgr_to_png_runs_frame(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, uint8_t* dst) {
    return png_code_host_frame(c, POPPY_FRAME_PNG_RUNS, bgr, stride, W, H, dst);
}
int poppy_hip_bgr_to_png_opt_frame(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, uint8_t* dst) {
    return png_code_host_frame(c, POPPY_FRAME_PNG_OPT, bgr, stride, W, H, dst);
}

// the length-build routine of k_png_opt_cost alone on given counts: what poppy_png_optimal_lengths gives, with its refusals
int poppy_hip_png_optimal_lengths(poppy_hip_ctx* c, const uint32_t* counts, int n_symbols, int limit, uint8_t* lengths) {
    if (!c) return POPPY_E_ARG;
    uint8_t host[png_opt::kSymbols];
    if (poppy_png_optimal_lengths(counts, n_symbols, limit, lengths ? host : nullptr) != POPPY_OK)      // (the refusals are the host statement's; its lengths are not used)
        return fail(c, POPPY_E_ARG, "bad arguments: a null pointer, n_symbols outside 1..286, a limit other than 7 or 15, counts that are all zero, whose sum is 2^32 or more, or more of them than 2^limit");
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t padded[png_opt::kSymbols] = {}, built[png_opt::kSymbols];
    memcpy(padded, counts, sizeof(uint32_t) * (size_t)n_symbols);
    CallBuffers held;
    uint8_t *d_counts = nullptr, *d_built = nullptr;
    HIPCHK(c, held.alloc(&d_counts, sizeof padded));
    HIPCHK(c, held.alloc(&d_built, sizeof built));
    hipError_t e = hipMemcpyAsync(d_counts, padded, sizeof padded, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch_png_length_build((const uint32_t*)d_counts, limit, (uint32_t*)d_built, c->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(built, d_built, sizeof built, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);     // nothing of the call is in flight when its buffers go (`held`, at the return)
    if (e == hipSuccess) e = e_sync;
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("PNG length build: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    for (int i = 0; i < n_symbols; ++i) {
        if (built[i] > (uint32_t)limit) return fail(c, POPPY_E_DEVICE, "a built length is outside its bounds");
        lengths[i] = (uint8_t)built[i];
    }
    return POPPY_OK;
}

// a host frame up (upload_host_bgr), the I444 kernel, the planes down, on buffers that live for the call
int poppy_hip_bgr_to_i444(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    if (!bgr || !dst || W <= 0 || H <= 0 || stride < (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = raster_bytes(kRasterI444, W, H);
    CallBuffers held;
    uint8_t *d_src = nullptr, *d_dst = nullptr;
    hipError_t e = held.alloc(&d_dst, bytes + 16);
    if (e == hipSuccess) e = upload_host_bgr(c, held, bgr, stride, W, H, &d_src);
    if (e == hipSuccess) { launch_bgr_to_i444(d_src, d_dst, W, H, c->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(dst, d_dst, bytes, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);     // nothing of the call is in flight when its buffers go (`held`, at the return)
    if (e == hipSuccess) e = e_sync;
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("BGR to I444: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

}  // extern "C"
