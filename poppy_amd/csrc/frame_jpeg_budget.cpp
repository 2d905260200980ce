// frame_jpeg_budget.cpp — POPPY_FRAME_JPEG and POPPY_FRAME_JPEG444 frames that fit a byte budget (include/poppy_hip.h, "JPEG byte budget", has the rule) in plain
// C++: the search over the qualities on a table (the search itself is written once, jpeg_tables.h: budget_search), the four host statements on top of frame_jpeg.cpp's coder, and poppy_jpeg_frame_quality,
// which reads a frame's quality back from its DQT.  kernels_frame_jpeg.hip (k_jpeg_measure, k_jpeg_pick) runs the same search on the device; the bytes are equal.
// Host only, integer arithmetic only.
#include "frame_limits.h"
#include <vector>

namespace poppy_hip {
namespace jpeg {

namespace {

// (the rule itself is jpeg_tables.h's budget_search; size(q) here: the JFIF file's length at quality q)
int planes_to_budget_frame(const uint8_t* planes, int width, int height, int quality_max, size_t budget, Sampling s, uint8_t* dst, int* quality_used) {
    if (!planes || !dst || width <= 0 || height <= 0 || quality_max < 1 || quality_max > 100 || budget == 0 || budget > 0xffffffffull) return POPPY_E_ARG;
    if (!jpeg_fits(width, height, s)) return POPPY_E_UNSUPPORTED;
    int in_dst = 0;                                         // the quality of the frame that stands in dst
    const int q = budget_search([&](int quality) { in_dst = quality; return encode_planes(planes, width, height, quality, s, dst) - 4; }, quality_max, budget);
    if (in_dst != q) encode_planes(planes, width, height, q, s, dst);
    if (quality_used) *quality_used = q;
    return POPPY_OK;
}

int bgr_to_budget_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality_max, size_t budget, Sampling s, uint8_t* dst, int* quality_used) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3 || quality_max < 1 || quality_max > 100 || budget == 0 || budget > 0xffffffffull) return POPPY_E_ARG;
    if (!jpeg_fits(width, height, s)) return POPPY_E_UNSUPPORTED;
    std::vector<uint8_t> planes(raster_bytes(s == k444 ? kRasterI444 : kRasterI420, (size_t)width, (size_t)height));
    const int rc = (s == k444 ? poppy_bgr_to_i444 : poppy_bgr_to_i420)(bgr, stride, width, height, planes.data());
    return rc ? rc : planes_to_budget_frame(planes.data(), width, height, quality_max, budget, s, dst, quality_used);
}

}  // namespace

}  // namespace jpeg
}  // namespace poppy_hip

extern "C" {

int poppy_jpeg_budget_pick(const uint32_t* sizes, int quality_max, size_t budget) {
    if (!sizes || quality_max < 1 || quality_max > 100 || budget == 0) return POPPY_E_ARG;
    return poppy_hip::jpeg::budget_search([&](int q) { return (size_t)sizes[q]; }, quality_max, budget);
}

int poppy_i420_to_jpeg_budget_frame(const uint8_t* i420, int width, int height, int quality_max, size_t budget, uint8_t* dst, int* quality_used) {
    return poppy_hip::jpeg::planes_to_budget_frame(i420, width, height, quality_max, budget, poppy_hip::jpeg::k420, dst, quality_used);
}
int poppy_i444_to_jpeg_budget_frame(const uint8_t* i444, int width, int height, int quality_max, size_t budget, uint8_t* dst, int* quality_used) {
    return poppy_hip::jpeg::planes_to_budget_frame(i444, width, height, quality_max, budget, poppy_hip::jpeg::k444, dst, quality_used);
}
int poppy_bgr_to_jpeg_budget_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality_max, size_t budget, uint8_t* dst, int* quality_used) {
    return poppy_hip::jpeg::bgr_to_budget_frame(bgr, stride, width, height, quality_max, budget, poppy_hip::jpeg::k420, dst, quality_used);
}
int poppy_bgr_to_jpeg444_budget_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality_max, size_t budget, uint8_t* dst, int* quality_used) {
    return poppy_hip::jpeg::bgr_to_budget_frame(bgr, stride, width, height, quality_max, budget, poppy_hip::jpeg::k444, dst, quality_used);
}

// the largest quality whose two tables are the frame's DQT entries (several qualities may share their tables: 1..100 are not 100 different pairs at the clamps)
int poppy_jpeg_frame_quality(const uint8_t* frame) {
    using namespace poppy_hip::jpeg;
    if (!frame || poppy_jpeg_frame_bytes(frame) < 4 + (size_t)kOffDqt + 130) return 0;
    const uint8_t* file = frame + 4;
    if (file[0] != 0xFF || file[1] != 0xD8 || file[kOffDqt - 4] != 0xFF || file[kOffDqt - 3] != 0xDB || file[kOffDqt] != 0 || file[kOffDqt + 65] != 1) return 0;
    for (int q = 100; q >= 1; --q) {
        bool same = true;
        for (int t = 0; t < 2 && same; ++t)
            for (int k = 0; k < 64 && same; ++k) same = file[kOffDqt + 65 * t + 1 + k] == (uint8_t)quant_entry(t, kZigzag[k], q);
        if (same) return q;
    }
    return 0;
}

}  // extern "C"
