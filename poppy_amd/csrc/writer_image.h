// writer_image.h — the frames that no slot renders, to the writer in its geometry and format: the phase 0 / 1 and t = 0 / 1 copies, the linear-blend fallback frames,
// host images.  Owns the context's scale and format scratch, and the stand-alone entry points that run one conversion kernel alone.  writer_image.cpp.
#pragma once
#include "frame_format.h"
#include <vector>

// a full-size device frame scaled down to g into c->scale_scratch on c->stream (grown when needed: the stream's order keeps the readers of one frame in front of
// the next frame's downscale)
int scale_into_scratch(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, const WriterGeom& g);
// a device frame (tight u8x3, W x H) in the writer's geometry g = context_geom(c, W, H) and format in `host`, queued on c->stream and waited for;
// *stride = what the writer is told
// n_copies: how often the writer gets this frame — under the sequence formats these copies are the whole sequence, and the frame is converted on the host
int download_frame(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, const WriterGeom& g, std::vector<uint8_t>& host, size_t* stride, int n_copies = 1);
const uint8_t* host_frame(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, std::vector<uint8_t>& tmp, size_t* out_stride, int* status, int n_copies = 1);      // a host frame (already in the writer's geometry) in the writer's format: `bgr` itself (BGR) or its I420 / PAL8 / coded form in `tmp`; nullptr, *status and c->err set, when the format refuses the frame
int write_device_image(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, int n_copies, poppy_write_cb write, void* user);      // a device image / a host image to the writer, n_copies times, in the writer's format (the phase 0 / 1 and t = 0 / 1 copies, the linear-blend fallback frames)
int write_host_image(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, int n_copies, poppy_write_cb write, void* user);
int jpeg_seq_of_copies(const uint8_t* bgr, size_t stride, int n_copies, int width, int height, int quality, int format, uint8_t* dst);      // frame_jpeg.cpp: the POPPY_FRAME_JPEG_SEQ / JPEG444_SEQ (`format`) frame of a sequence that is n_copies times the same BGR frame: its counts n_copies times in the sums, one frame out
int jpeg_seq_budget_of_copies(const uint8_t* bgr, size_t stride, int n_copies, int width, int height, int quality_max, uint64_t budget, int format, uint8_t* dst);      // frame_jpeg_seq_budget.cpp: the POPPY_FRAME_JPEG / JPEG444 (`format`) frame of a sequence under a sequence budget that is n_copies times the same BGR frame: its size n_copies times in the sums, one frame out
int png_seq_of_copies(const uint8_t* bgr, size_t stride, int n_copies, int width, int height, uint8_t* dst);      // frame_png_seq.cpp: the POPPY_FRAME_PNG_SEQ frame of a sequence that is n_copies times the same BGR frame: its counts n_copies times in the sums, one frame out
int pal8_seq_of_copies(const uint8_t* bgr, size_t stride, int n_copies, int width, int height, uint8_t* dst);      // frame_pal8.cpp: the POPPY_FRAME_PAL8_SEQ frame of a sequence that is n_copies times the same BGR frame (poppy_bgr_frames_to_pal8 with frame_stride 0, one frame out)
