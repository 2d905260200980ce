// frame_jpeg_seq_budget.cpp — POPPY_FRAME_JPEG and POPPY_FRAME_JPEG444 frames of a sequence that fit one byte budget together, all at one quality
// (include/poppy_hip.h, "JPEG sequence budget", has the rule) in plain C++: the per-frame budget's search (jpeg_tables.h: budget_search) on size(q), the sum of
// every frame's file at quality q, and the four host statements on top of frame_jpeg.cpp's coder.  kernels_frame_jpeg.hip (k_jpeg_measure over a store of frames,
// k_jpeg_pick in its sequence form) runs the same search on the device; the bytes are equal.  Host only, integer arithmetic only.
#include "frame_limits.h"
#include <vector>

namespace poppy_hip {
namespace jpeg {

namespace {

// the refusals, all from the arguments alone.  A sequence's worst case always fits 64-bit sums — a frame's capacity is below 2^32 (jpeg_fits) and the frame count
// is an int, so size(q) stays below 2^63 —: there is no limit on the sequence beyond the frames' own.
int seq_budget_refuses(const void* src, const void* dst, size_t frame_stride, size_t frame_bytes, int n_frames, int width, int height, int quality_max, uint64_t budget, Sampling s) {
    if (!src || !dst || n_frames < 1 || width <= 0 || height <= 0 || frame_stride < frame_bytes || quality_max < 1 || quality_max > 100 || budget == 0) return POPPY_E_ARG;
    return jpeg_fits(width, height, s) ? POPPY_OK : POPPY_E_UNSUPPORTED;
}

// n frames of planes frame_stride bytes apart, every frame standing for `copies` of itself in the sum; frame k at the picked quality goes to dst + k * dst_stride
int encode_planes_seq_budget(const uint8_t* planes, size_t frame_stride, int n, int copies, int w, int h, int quality_max, uint64_t budget, Sampling s, uint8_t* dst, size_t dst_stride) {
    std::vector<uint8_t> tmp((size_t)frame_capacity((size_t)w, (size_t)h, s));
    const int q = budget_search([&](int quality) {
        unsigned long long sum = 0;
        for (int k = 0; k < n; ++k) sum += (unsigned long long)(encode_planes(planes + (size_t)k * frame_stride, w, h, quality, s, tmp.data()) - 4) * (unsigned long long)copies;
        return sum;
    }, quality_max, budget);
    for (int k = 0; k < n; ++k) encode_planes(planes + (size_t)k * frame_stride, w, h, q, s, dst + (size_t)k * dst_stride);
    return q;
}

int planes_to_seq_budget(const uint8_t* planes, size_t frame_stride, int n_frames, int width, int height, int quality_max, uint64_t budget, Sampling s, uint8_t* dst, int* quality_used) {
    if (width <= 0 || height <= 0) return POPPY_E_ARG;
    if (const int rc = seq_budget_refuses(planes, dst, frame_stride, raster_bytes(s == k444 ? kRasterI444 : kRasterI420, (size_t)width, (size_t)height), n_frames, width, height, quality_max, budget, s)) return rc;
    const int q = encode_planes_seq_budget(planes, frame_stride, n_frames, 1, width, height, quality_max, budget, s, dst, (size_t)frame_capacity((size_t)width, (size_t)height, s));
    if (quality_used) *quality_used = q;
    return POPPY_OK;
}

int bgr_frames_to_seq_budget(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality_max, uint64_t budget, Sampling s, uint8_t* dst, int* quality_used) {
    if (width <= 0 || height <= 0 || stride < (size_t)width * 3) return POPPY_E_ARG;
    if (const int rc = seq_budget_refuses(bgr, dst, frame_stride, stride * ((size_t)height - 1) + (size_t)width * 3, n_frames, width, height, quality_max, budget, s)) return rc;
    const size_t place = raster_bytes(s == k444 ? kRasterI444 : kRasterI420, (size_t)width, (size_t)height);
    std::vector<uint8_t> planes(place * (size_t)n_frames);
    for (int k = 0; k < n_frames; ++k)
        if (const int rc = (s == k444 ? poppy_bgr_to_i444 : poppy_bgr_to_i420)(bgr + (size_t)k * frame_stride, stride, width, height, planes.data() + (size_t)k * place)) return rc;
    return planes_to_seq_budget(planes.data(), place, n_frames, width, height, quality_max, budget, s, dst, quality_used);
}

}  // namespace

}  // namespace jpeg
}  // namespace poppy_hip

extern "C" {

int poppy_i420_frames_to_jpeg_seq_budget_frames(const uint8_t* i420, size_t frame_stride, int n_frames, int width, int height, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used) {
    return poppy_hip::jpeg::planes_to_seq_budget(i420, frame_stride, n_frames, width, height, quality_max, budget, poppy_hip::jpeg::k420, dst, quality_used);
}
int poppy_i444_frames_to_jpeg_seq_budget_frames(const uint8_t* i444, size_t frame_stride, int n_frames, int width, int height, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used) {
    return poppy_hip::jpeg::planes_to_seq_budget(i444, frame_stride, n_frames, width, height, quality_max, budget, poppy_hip::jpeg::k444, dst, quality_used);
}
int poppy_bgr_frames_to_jpeg_seq_budget_frames(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used) {
    return poppy_hip::jpeg::bgr_frames_to_seq_budget(bgr, stride, frame_stride, n_frames, width, height, quality_max, budget, poppy_hip::jpeg::k420, dst, quality_used);
}
int poppy_bgr_frames_to_jpeg444_seq_budget_frames(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used) {
    return poppy_hip::jpeg::bgr_frames_to_seq_budget(bgr, stride, frame_stride, n_frames, width, height, quality_max, budget, poppy_hip::jpeg::k444, dst, quality_used);
}

}  // extern "C"

// writer_image.h: a sequence that is n_copies times the same frame; that frame once in dst
int jpeg_seq_budget_of_copies(const uint8_t* bgr, size_t stride, int n_copies, int width, int height, int quality_max, uint64_t budget, int format, uint8_t* dst) {
    using namespace poppy_hip::jpeg;
    const Sampling s = format == POPPY_FRAME_JPEG444 ? k444 : k420;
    if (width <= 0 || height <= 0 || stride < (size_t)width * 3) return POPPY_E_ARG;
    if (const int rc = seq_budget_refuses(bgr, dst, 0, 0, n_copies, width, height, quality_max, budget, s)) return rc;
    std::vector<uint8_t> planes(raster_bytes(s == k444 ? kRasterI444 : kRasterI420, (size_t)width, (size_t)height));
    if (const int rc = (s == k444 ? poppy_bgr_to_i444 : poppy_bgr_to_i420)(bgr, stride, width, height, planes.data())) return rc;
    encode_planes_seq_budget(planes.data(), 0, 1, n_copies, width, height, quality_max, budget, s, dst, 0);
    return POPPY_OK;
}
