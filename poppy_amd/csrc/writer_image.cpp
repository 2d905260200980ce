// writer_image.cpp — the frames that no slot renders (writer_image.h): a device or host image scaled and converted for the writer on the context's stream, and the
// stand-alone entry points that run one conversion kernel alone on buffers that live for the call.
#include "context.h"

int scale_into_scratch(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, const WriterGeom& g) {
    HIPCHK(c, c->scale_scratch.reserve(poppy_frame_bytes(POPPY_FRAME_BGR, g.w, g.h) + 16, c->stream));      // (the stream may still read the buffer that growth frees)
    launch_writer_scaling(g, d_bgr, c->scale_scratch.p, W, H, c->stream);
    HIPCHK(c, hipGetLastError());
    return POPPY_OK;
}

// a PAL8 frame in device memory -> its POPPY_FRAME_GIF frame in `host` (exactly `total` bytes), on the context's stream and waited for: the frames that no slot renders,
// and poppy_hip_pal8_to_gif_frame.  The buffers live for the call.
static int gif_from_device_pal8(poppy_hip_ctx* c, const uint8_t* d_pal8, int W, int H, std::vector<uint8_t>& host) {
    const size_t cap = poppy_frame_bytes(POPPY_FRAME_GIF, W, H);
    CallBuffers held;
    uint8_t *work = nullptr, *frame = nullptr;
    hipError_t e = held.alloc(&work, gif_scratch_bytes(W, H));
    if (e == hipSuccess) e = held.alloc(&frame, cap + 16);
    uint32_t total = 0;
    if (e == hipSuccess) {
        enqueue_gif_coding(d_pal8, work, frame, nullptr, W, H, c->stream, nullptr, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&total, frame, 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && !coded_length_ok(total, cap)) return fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds");
    if (e == hipSuccess) { host.resize(total); e = hipMemcpy(host.data(), frame, total, hipMemcpyDeviceToHost); }
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); c->err = std::string("GIF frame coding: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

// an I420 frame in device memory -> its POPPY_FRAME_JPEG frame in `host` (exactly `total` bytes) at the quality that `d_tables` name, on the context's stream and
// waited for: the frames that no slot renders, and poppy_hip_i420_to_jpeg_frame.  The buffers live for the call.  sm == k444: an I444 frame -> its
// POPPY_FRAME_JPEG444 frame (poppy_hip_i444_to_jpeg_frame).
static int jpeg_from_device_planes(poppy_hip_ctx* c, const uint8_t* d_i420, const void* d_tables, int W, int H, jpeg::Sampling sm, std::vector<uint8_t>& host) {
    const size_t cap = jpeg_frame_capacity((size_t)W, (size_t)H, sm);
    CallBuffers held;
    uint8_t *work = nullptr, *frame = nullptr;
    hipError_t e = held.alloc(&work, jpeg_scratch_bytes(W, H, sm));
    if (e == hipSuccess) e = held.alloc(&frame, cap + 16);
    uint32_t total = 0;
    if (e == hipSuccess) {
        enqueue_jpeg_coding(d_i420, d_tables, work, frame, nullptr, W, H, sm, c->stream, nullptr, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&total, frame, 4, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);     // nothing of the call is in flight when its buffers go
    if (e == hipSuccess) e = e_sync;
    if (e == hipSuccess && !coded_length_ok(total, cap, kJpegFrameMinBytes)) return fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds");
    if (e == hipSuccess) { host.resize(total); e = hipMemcpy(host.data(), frame, total, hipMemcpyDeviceToHost); }
    if (e != hipSuccess) { c->err = std::string("JPEG frame coding: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

// a tight BGR frame in device memory -> its POPPY_FRAME_PNG or POPPY_FRAME_PNG_RUNS frame (fmt) in `host` (exactly `total` bytes), on the context's stream and waited
// for: the frames that no slot renders, and poppy_hip_bgr_to_png_frame, poppy_hip_bgr_to_png_runs_frame.  The buffers live for the call, at fmt's capacity.
static int png_from_device_bgr(poppy_hip_ctx* c, int fmt, const uint8_t* d_bgr, int W, int H, std::vector<uint8_t>& host) {
    const size_t cap = png_frame_capacity(fmt, (size_t)W, (size_t)H);
    CallBuffers held;
    uint8_t *work = nullptr, *frame = nullptr;
    hipError_t e = held.alloc(&work, png_scratch_bytes(W, H, fmt == POPPY_FRAME_PNG_RUNS));
    if (e == hipSuccess) e = held.alloc(&frame, cap + 16);
    uint32_t total = 0;
    if (e == hipSuccess) {
        enqueue_png_coding(fmt, d_bgr, work, frame, nullptr, W, H, c->stream, nullptr, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&total, frame, 4, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);     // nothing of the call is in flight when its buffers go
    if (e == hipSuccess) e = e_sync;
    if (e == hipSuccess && !coded_length_ok(total, cap, kPngFrameMinBytes)) return fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds");
    if (e == hipSuccess) { host.resize(total); e = hipMemcpy(host.data(), frame, total, hipMemcpyDeviceToHost); }
    if (e != hipSuccess) { c->err = std::string("PNG frame coding: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

int download_frame(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, const WriterGeom& g, std::vector<uint8_t>& host, size_t* stride, int n_copies) {
    const int fmt = c->frame_format;
    if (const char* why = format_refuses(fmt, g.w, g.h)) return fail(c, POPPY_E_UNSUPPORTED, why);
    if (g.scaled()) {                                              // scaled first, on the device; everything below is in the writer's geometry
        int rc = scale_into_scratch(c, d_bgr, W, H, g); if (rc) return rc;
        d_bgr = c->scale_scratch.p; W = g.w; H = g.h;
    }
    if (format_is_sequence(fmt)) {                                 // the copies are the sequence: the host statement on the BGR frame
        std::vector<uint8_t> bgr((size_t)W * H * 3);
        HIPCHK(c, hipMemcpyAsync(bgr.data(), d_bgr, bgr.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        int rc = POPPY_OK;
        const uint8_t* frame = host_frame(c, bgr.data(), (size_t)W * 3, W, H, host, stride, &rc, n_copies);
        return frame ? POPPY_OK : rc;
    }
    *stride = writer_stride(fmt, W);
    const uint8_t* d_frame = d_bgr;
    if (fmt != POPPY_FRAME_BGR) {                                  // converted into the context's scratch: the slots' launches on other buffers
        // (a coded format: its raster form into the scratch — PAL8 for GIF, I420 for JPEG, the I444 planes for JPEG444 —, then the coder on buffers that live for the call)
        if (format_is_png(fmt)) return png_from_device_bgr(c, fmt, d_bgr, W, H, host);      // (no raster form: the coder reads the BGR frame)
        if (fmt == POPPY_FRAME_JPEG444) {                          // (I444 is no format of its own: the kernel is launched here)
            { int rc = ensure_jpeg_tables(c); if (rc) return rc; }
            HIPCHK(c, c->fmt_scratch.reserve((size_t)W * H * 3 + 16, c->stream));
            launch_bgr_to_i444(d_bgr, c->fmt_scratch.p, W, H, c->stream);
            HIPCHK(c, hipGetLastError());
            return jpeg_from_device_planes(c, c->fmt_scratch.p, c->jpeg_tables, W, H, jpeg::k444, host);
        }
        const bool gif = fmt == POPPY_FRAME_GIF, jpeg = fmt == POPPY_FRAME_JPEG;
        const int raster = gif ? POPPY_FRAME_PAL8 : jpeg ? POPPY_FRAME_I420 : fmt;
        if (format_builds_palette(fmt)) { int rc = alloc_zeroed_tables(c, &c->fmt_scratch_tables, kPal8TableBytes); if (rc) return rc; }
        if (jpeg) { int rc = ensure_jpeg_tables(c); if (rc) return rc; }
        HIPCHK(c, c->fmt_scratch.reserve(poppy_frame_bytes(raster, W, H) + 16, c->stream));
        SlotFormat scratch;
        scratch.i420 = scratch.pal8 = c->fmt_scratch.p; scratch.pal8_tables = c->fmt_scratch_tables;
        enqueue_conversion(raster, WriterGeom{W, H}, d_bgr, W, H, scratch, c->stream, nullptr, nullptr);
        HIPCHK(c, hipGetLastError());
        if (gif) return gif_from_device_pal8(c, c->fmt_scratch.p, W, H, host);
        if (jpeg) return jpeg_from_device_planes(c, c->fmt_scratch.p, c->jpeg_tables, W, H, jpeg::k420, host);
        d_frame = c->fmt_scratch.p;
    }
    host.resize(poppy_frame_bytes(fmt, W, H));
    HIPCHK(c, hipMemcpyAsync(host.data(), d_frame, host.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return POPPY_OK;
}

const uint8_t* host_frame(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, std::vector<uint8_t>& tmp, size_t* out_stride, int* status, int n_copies) {
    const int fmt = c->frame_format;
    *out_stride = stride;
    *status = POPPY_OK;
    if (fmt == POPPY_FRAME_BGR) return bgr;
    if (const char* why = format_refuses(fmt, W, H)) { *status = fail(c, POPPY_E_UNSUPPORTED, why); return nullptr; }
    tmp.resize(poppy_frame_bytes(fmt, W, H));
    std::vector<uint8_t> pal8(format_is_sequence(fmt) && format_is_coded(fmt) ? poppy_frame_bytes(POPPY_FRAME_PAL8_SEQ, W, H) : 0);      // (GIF_SEQ: PAL8_SEQ's frame, then the host coder)
    int rc = format_is_sequence(fmt) ? pal8_seq_of_copies(bgr, stride, std::max(1, n_copies), W, H, pal8.empty() ? tmp.data() : pal8.data()) :
                   fmt == POPPY_FRAME_GIF ? poppy_bgr_to_gif_frame(bgr, stride, W, H, tmp.data()) :
                   fmt == POPPY_FRAME_JPEG ? poppy_bgr_to_jpeg_frame(bgr, stride, W, H, c->jpeg_quality, tmp.data()) :
                   fmt == POPPY_FRAME_JPEG444 ? poppy_bgr_to_jpeg444_frame(bgr, stride, W, H, c->jpeg_quality, tmp.data()) :
                   fmt == POPPY_FRAME_PNG ? poppy_bgr_to_png_frame(bgr, stride, W, H, tmp.data()) :
                   fmt == POPPY_FRAME_PNG_RUNS ? poppy_bgr_to_png_runs_frame(bgr, stride, W, H, tmp.data()) :
                   fmt == POPPY_FRAME_PAL8 ? poppy_bgr_to_pal8(bgr, stride, W, H, tmp.data()) : poppy_bgr_to_i420(bgr, stride, W, H, tmp.data());
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

// the body of the two stand-alone scaling entries: a host frame W x H up, scaled to g on the device, down again, on buffers that live for the call.  The source's
// place behind a 256-byte boundary is the row pad's low bits (include/poppy_hip.h).
static int scale_host_frame(poppy_hip_ctx* c, const char* what, const uint8_t* bgr, size_t stride, int W, int H, const WriterGeom& g, uint8_t* dst, size_t dst_stride) {
    HIPCHK(c, hipSetDevice(c->device));
    const size_t row = (size_t)W * 3, shift = (stride - row) % 16, out_row = (size_t)g.w * 3;
    CallBuffers held;
    uint8_t *d_src = nullptr, *d_dst = nullptr;
    hipError_t e = held.alloc(&d_src, row * H + shift + 16);
    if (e == hipSuccess) e = held.alloc(&d_dst, out_row * g.h + 16);
    if (e == hipSuccess) e = copy_rows_async(d_src + shift, row, bgr, stride, row, (size_t)H, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch_writer_scaling(g, d_src + shift, d_dst, W, H, c->stream); e = hipGetLastError(); }
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
    CallBuffers held;                                              // (gif_from_device_pal8 waits for the stream before it returns)
    uint8_t* d_pal8 = nullptr;
    HIPCHK(c, held.alloc(&d_pal8, bytes + 16));
    if (hipMemcpy(d_pal8, pal8, bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(c, POPPY_E_DEVICE, "upload of the PAL8 frame failed");
    std::vector<uint8_t> host;
    const int rc = gif_from_device_pal8(c, d_pal8, W, H, host);
    if (rc == POPPY_OK) memcpy(dst, host.data(), host.size());
    return rc;
}

// the body of poppy_hip_i420_to_jpeg_frame and poppy_hip_i444_to_jpeg_frame: the planes of format `fmt`'s sampling up, the two kernels, `total` bytes down
static int jpeg_code_host_planes(poppy_hip_ctx* c, int fmt, const uint8_t* i420, int W, int H, int quality, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    if (!i420 || !dst || W <= 0 || H <= 0 || quality < 1 || quality > 100) return fail(c, POPPY_E_ARG, "bad arguments");
    if (const char* why = format_refuses(fmt, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = fmt == POPPY_FRAME_JPEG444 ? (size_t)W * H * 3 : poppy_frame_bytes(POPPY_FRAME_I420, W, H);
    jpeg::QualityTables t;
    jpeg::fill_quality_tables(quality, &t);
    CallBuffers held;                                              // (jpeg_from_device_planes waits for the stream before it returns)
    uint8_t *d_i420 = nullptr, *d_tables = nullptr;
    HIPCHK(c, held.alloc(&d_i420, bytes + 16));
    HIPCHK(c, held.alloc(&d_tables, kJpegTableBytes));
    if (hipMemcpy(d_i420, i420, bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_tables, &t, sizeof t, hipMemcpyHostToDevice) != hipSuccess)
        return fail(c, POPPY_E_DEVICE, "upload of the planes failed");
    std::vector<uint8_t> host;
    const int rc = jpeg_from_device_planes(c, d_i420, d_tables, W, H, format_sampling(fmt), host);
    if (rc == POPPY_OK) memcpy(dst, host.data(), host.size());
    return rc;
}

int poppy_hip_i420_to_jpeg_frame(poppy_hip_ctx* c, const uint8_t* i420, int W, int H, int quality, uint8_t* dst) {
    return jpeg_code_host_planes(c, POPPY_FRAME_JPEG, i420, W, H, quality, dst);
}

int poppy_hip_i444_to_jpeg_frame(poppy_hip_ctx* c, const uint8_t* i444, int W, int H, int quality, uint8_t* dst) {
    return jpeg_code_host_planes(c, POPPY_FRAME_JPEG444, i444, W, H, quality, dst);
}

// a host frame up, the six PNG kernels, `total` bytes down, on buffers that live for the call; the source's place behind a 256-byte boundary is the row pad's low
// bits (include/poppy_hip.h), as in scale_host_frame
static int png_code_host_frame(poppy_hip_ctx* c, int fmt, const uint8_t* bgr, size_t stride, int W, int H, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    if (!bgr || !dst || W <= 0 || H <= 0 || stride < (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad arguments");
    if (const char* why = format_refuses(fmt, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t row = (size_t)W * 3, shift = (stride - row) % 16;
    CallBuffers held;                                              // (png_from_device_bgr waits for the stream before it returns)
    uint8_t* d_src = nullptr;
    HIPCHK(c, held.alloc(&d_src, row * H + shift + 16));
    if (copy_rows_async(d_src + shift, row, bgr, stride, row, (size_t)H, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return fail(c, POPPY_E_DEVICE, "upload of the BGR frame failed");
    }
    std::vector<uint8_t> host;
    const int rc = png_from_device_bgr(c, fmt, d_src + shift, W, H, host);
    if (rc == POPPY_OK) memcpy(dst, host.data(), host.size());
    return rc;
}
int poppy_hip_bgr_to_png_frame(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, uint8_t* dst) {
    return png_code_host_frame(c, POPPY_FRAME_PNG, bgr, stride, W, H, dst);
}
int poppy_hip_bgr_to_png_runs_frame(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, uint8_t* dst) {
    return png_code_host_frame(c, POPPY_FRAME_PNG_RUNS, bgr, stride, W, H, dst);
}

// a host frame up, the I444 kernel, the planes down, on buffers that live for the call; the source's place behind a 256-byte boundary is the row pad's low bits
// (include/poppy_hip.h), as in scale_host_frame
int poppy_hip_bgr_to_i444(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    if (!bgr || !dst || W <= 0 || H <= 0 || stride < (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t row = (size_t)W * 3, shift = (stride - row) % 16, bytes = row * H;
    CallBuffers held;
    uint8_t *d_src = nullptr, *d_dst = nullptr;
    hipError_t e = held.alloc(&d_src, bytes + shift + 16);
    if (e == hipSuccess) e = held.alloc(&d_dst, bytes + 16);
    if (e == hipSuccess) e = copy_rows_async(d_src + shift, row, bgr, stride, row, (size_t)H, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch_bgr_to_i444(d_src + shift, d_dst, W, H, c->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(dst, d_dst, bytes, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);     // nothing of the call is in flight when its buffers go (`held`, at the return)
    if (e == hipSuccess) e = e_sync;
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("BGR to I444: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

}  // extern "C"
