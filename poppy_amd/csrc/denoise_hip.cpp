// denoise_hip.cpp — the non-local-means denoise on a context (include/poppy_hip.h: poppy_hip_denoise): the weight table's way to the device, the two entry
// points and the list's setting.  The table and its constants come from poppy_denoise_weights (denoise.cpp) and from nowhere else; the kernel:
// kernels_denoise.hip.
#include "context.h"
#include "denoise.h"

using namespace poppy_denoise;

namespace {

// the refusals of every entry point, in the host statement's order; nothing is allocated or launched behind one
int refuse(poppy_hip_ctx* c, bool pointers_and_sizes_ok, float hs, int tw, int sw) {
    if (!pointers_and_sizes_ok) return fail(c, POPPY_E_ARG, "denoise: bad image arguments");
    const char* why = nullptr;
    const int rc = check_params(hs, tw, sw, &why);
    return rc ? fail(c, rc, why) : POPPY_OK;
}

// t[0 .. L) of (hs, tw, sw) on the device.  A change of parameters waits for the stream first: a queued launch may still read the table that is replaced.
int ensure_table(poppy_hip_ctx* c, float hs, int tw, int sw) {
    poppy_hip_ctx::Denoise& d = c->denoise;
    if (d.table.p && d.table_hs == hs && d.table_tw == tw && d.table_sw == sw) return POPPY_OK;
    std::vector<uint32_t> t((size_t)kMaxTable);
    int n = 0, L = 0, shift = 0; uint32_t fpm = 0;
    const int rc = poppy_denoise_weights(hs, tw, sw, t.data(), (int)t.size(), &n, &L, &fpm, &shift);
    if (rc) return fail(c, rc, "denoise: the weight table");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    d.table_hs = 0;
    HIPCHK(c, d.table.reserve((size_t)L * 4));
    HIPCHK(c, hipMemcpy(d.table.p, t.data(), (size_t)L * 4, hipMemcpyHostToDevice));
    d.table_hs = hs; d.table_tw = tw; d.table_sw = sw; d.L = L; d.shift = shift;
    return POPPY_OK;
}

}  // namespace

int denoise_queue(poppy_hip_ctx* c, const uint8_t* d_src, size_t stride, uint8_t* d_dst, int w, int h, float hs, int tw, int sw) {
    const int rc = ensure_table(c, hs, tw, sw); if (rc) return rc;
    const poppy_hip_ctx::Denoise& d = c->denoise;
    HIPCHK(c, launch_denoise(d_src, stride, d_dst, w, h, tw, sw, d.shift, d.L, (const uint32_t*)d.table.p, c->stream));
    return POPPY_OK;
}

extern "C" {

int poppy_hip_denoise(poppy_hip_ctx* c, const uint8_t* src, size_t stride, int w, int h, float hs, int tw, int sw, uint8_t* dst, size_t dst_stride) {
    if (!c) return POPPY_E_ARG;
    int rc = refuse(c, src && dst && w > 0 && h > 0 && stride >= (size_t)w * 3 && dst_stride >= (size_t)w * 3, hs, tw, sw); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t B = (size_t)w * h * 3;
    HIPCHK(c, c->denoise.stage.reserve(2 * B, c->stream));
    uint8_t *d_src = c->denoise.stage.p, *d_dst = d_src + B;
    HIPCHK(c, copy_rows_async(d_src, (size_t)w * 3, src, stride, (size_t)w * 3, h, hipMemcpyHostToDevice, c->stream));
    rc = denoise_queue(c, d_src, (size_t)w * 3, d_dst, w, h, hs, tw, sw);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }          // the upload reads src
    const hipError_t e = copy_rows_async(dst, dst_stride, d_dst, (size_t)w * 3, (size_t)w * 3, h, hipMemcpyDeviceToHost, c->stream);
    const hipError_t synced = hipStreamSynchronize(c->stream);
    HIPCHK(c, e);
    HIPCHK(c, synced);
    return POPPY_OK;
}

int poppy_hip_denoise_device(poppy_hip_ctx* c, const uint8_t* d_src, uint8_t* d_dst, int w, int h, float hs, int tw, int sw) {
    if (!c) return POPPY_E_ARG;
    const int rc = refuse(c, d_src && d_dst && d_src != d_dst && w > 0 && h > 0, hs, tw, sw); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return denoise_queue(c, d_src, (size_t)w * 3, d_dst, w, h, hs, tw, sw);
}

int poppy_hip_set_denoise(poppy_hip_ctx* c, float hs, int tw, int sw) {
    if (!c) return POPPY_E_ARG;
    if (hs == 0.0f) { c->denoise.hs = 0; c->denoise.tw = c->denoise.sw = 0; return POPPY_OK; }
    const int rc = refuse(c, true, hs, tw, sw); if (rc) return rc;
    c->denoise.hs = hs; c->denoise.tw = tw; c->denoise.sw = sw;
    return POPPY_OK;
}

int poppy_hip_get_denoise(poppy_hip_ctx* c, float* hs, int* tw, int* sw) {
    if (!c || !hs || !tw || !sw) return POPPY_E_ARG;
    *hs = c->denoise.hs; *tw = c->denoise.tw; *sw = c->denoise.sw;
    return POPPY_OK;
}

}  // extern "C"
