// frame_format.h — what depends on the format a writer gets its frames in (poppy_hip_set_frame_format) and on the writer's geometry (poppy_hip_set_frame_scale,
// poppy_hip_set_frame_size): the formats' facts, WriterGeom, a slot's conversion buffers and the conversion launches.  frame_format.cpp.  The palette sequence is
// palette_seq.h's, the pinned ring towards the writer writer_ring.h's, the frames that no slot renders writer_image.h's.
#pragma once
#include "../../include/poppy_hip.h"
#include <hip/hip_runtime.h>
#include "frame_limits.h"
#include "kernels.h"

struct poppy_hip_ctx; struct FrameSlot; struct Timer;

// The formats' facts are frame_limits.h's records (format_traits: raster form, coder, sequence, the smallest `total`); a context's format is always a known one
// (poppy_hip_set_frame_format refuses the others), so the functions below that take `fmt` read its record without asking.
const char* format_refuses(int fmt, int W, int H);      // why `fmt` refuses a W x H frame, or null: checked on the arguments alone, before anything is allocated or any state changes
size_t writer_stride(int fmt, int W);      // what the writer is told (format_stride): 0 for a coded frame, the width for the planar and palette formats, 3 * width for BGR
// The writer's geometry: what a W x H frame is for the writer of a context — ow x oh.  Under a scale s (poppy_hip_set_frame_scale) ow = (W + s - 1) / s,
// oh = (H + s - 1) / s (kScaleFactor); under a size (poppy_hip_set_frame_size) ow x oh is that size (kScaleSize); a context has at most one of the two.
// Everything the writer sees is sized by it: strides, frame bytes, the pinned ring, the conversion buffers, the formats' limits, the sequence store.
// Frames kept on the device (no writer) have kScaleNone: the pair's own geometry.
enum ScaleKind { kScaleNone = 0, kScaleFactor = 1, kScaleSize = 2 };
struct WriterGeom {
    int w = 0, h = 0, scale = 1;
    int kind = kScaleNone;
    bool scaled() const { return kind != kScaleNone; }
    bool operator==(const WriterGeom& o) const { return w == o.w && h == o.h && scale == o.scale && kind == o.kind; }
    bool operator!=(const WriterGeom& o) const { return !(*this == o); }
};
WriterGeom scaled_geom(int W, int H, int scale);
WriterGeom sized_geom(int ow, int oh);
WriterGeom context_geom(const poppy_hip_ctx* c, int W, int H, bool has_writer = true);      // of a W x H frame under the context's scale or size (which W x H admits: writer_refuses)
WriterGeom writer_geom(const poppy_hip_ctx* c, bool has_writer = true);      // of the resident pair's frames
const char* writer_refuses(const poppy_hip_ctx* c, int fmt, int W, int H);      // why a W x H frame cannot go to a writer under the context's scale or size in format `fmt`, or null: the size's admission, then format_refuses on the writer's geometry
void launch_writer_scaling(const WriterGeom& g, const uint8_t* src, uint8_t* dst, int W, int H, hipStream_t s, hipEvent_t done = nullptr);      // W x H -> g on the device (g.scaled()): the whole-factor downscale or the area resize
const char* scaling_mark(const WriterGeom& g);      // its name in timing mode 1: frame_scale or frame_resize
int writer_format(const poppy_hip_ctx* c, bool has_writer);      // the format of the frames a call hands to its writer (none: they stay BGR in HBM), and whether they are collected into one palette sequence first
bool writer_wants_sequence(const poppy_hip_ctx* c, bool has_writer);
// The record of format `fmt` as the context's writer gets it: the format's own, except that under a sequence budget (poppy_hip_set_jpeg_sequence_budget) POPPY_FRAME_JPEG
// and POPPY_FRAME_JPEG444 are held back as a sequence — the same frames, capacity and smallest frame on the Annex K tables, `sequence` set: no slot converts or
// codes them, the sequence pass stores their planes and the sequence's search and coder do the rest (palette_seq.h).
const FormatTraits& writer_traits(const poppy_hip_ctx* c, int fmt);
const char* sequence_refuses(int fmt, int n, int W, int H);      // ... and why a sequence of n such frames is refused, or null

struct SlotFormat {
    uint8_t* scaled = nullptr;            // a scale above 1 or a size: the frame scaled down, tight BGR, ow x oh — what the conversion reads and, under BGR, what the writer gets
    uint8_t* i420 = nullptr;              // the frame in the raster form of the format's record (raster_bytes): for the writer, or what the format's coder reads.  Allocated
    uint8_t* i444 = nullptr;              // when a format with that raster step is set and a pair is there; kept until the pair's buffers go
    uint8_t* pal8 = nullptr;              // ... and the PAL8 conversion's tables (kernels.h: kPal8TableBytes) — the slot's own, because the conversions of frames in
    uint8_t* pal8_tables = nullptr;       // flight run beside each other (allocated like the raster buffers; the stream and event live as long as the context)
    uint8_t* coded = nullptr;             // a format with a coder step: the coded frame for the writer (its capacity: poppy_frame_bytes), the coder's scratch
    uint8_t* coded_scratch = nullptr;     // (coding_scratch_bytes) and a word of mapped pinned memory that the coder's last kernel stores the frame's length into: the host
    uint32_t* coded_total = nullptr;      // reads it when `done` has fired and copies that many bytes; the three
    void* coded_total_dev = nullptr;      // are sized by coded_for, the format they were allocated under, and allocated again when the context's coded format is another
    int coded_for = POPPY_FRAME_BGR;
    const void* jpeg_tables = nullptr;    // the JPEG coder: the context's tables for its quality (ensure_jpeg_tables; the context's to free)
    poppy_hip::JpegBudget jpeg_budget;    // ... and, with a byte budget set (poppy_hip_set_jpeg_budget), the context's tables of all qualities and the budget's words (context_jpeg_budget); empty: off
    hipStream_t fmt_stream = nullptr;     // chained PAL8 / PAL8_SEQ frames: the conversion's side stream (the chain goes on from the unsharp: enqueue_body)
    hipEvent_t bgr_done = nullptr;        // ... and the event that rides on that unsharp
};
int alloc_slot_format(poppy_hip_ctx* c);          // every slot's buffers for the context's format and the pair's geometry: allocates what is missing
void free_slot_format_pair(SlotFormat& f);        // what goes with the pair's buffers
void free_slot_format_ctx(SlotFormat& f);         // the side stream and its event: they live as long as the context
void free_context_format(poppy_hip_ctx* c);       // the context's own: scratch of the frames that no slot renders, the sequence's tables, store and rings
bool slot_format_ready(const poppy_hip_ctx* c, const FrameSlot& f, int fmt, const WriterGeom& g);      // (every way to a format with a pair allocates the slots' buffers — alloc_pair, poppy_hip_set_frame_format — or refuses: a frame is never converted into nothing)
const uint8_t* slot_frame(const FrameSlot& f, int fmt, const WriterGeom& g);       // the slot's frame as the writer gets it
const uint8_t* slot_bgr(const FrameSlot& f, const WriterGeom& g);       // ... and as BGR in the writer's geometry: the frame itself, or the scaled frame
bool slot_frame_length(const FrameSlot& f, int fmt, size_t capacity, size_t* bytes);      // the bytes of that frame, once its `done` has fired: `capacity`, or a coded frame's own length from the slot's pinned word; false when that is out of bounds

// src_bgr (W x H) scaled down to g into b.scaled (g.scaled(): the first dispatch) and in format `fmt` into b's buffers on stream s, in the two steps of the
// format's record: the raster step (enqueue_raster), then the coder step (enqueue_coding) on what it wrote, on the context's tables (b.jpeg_tables) under JPEG.
// `done` (optional) rides on the last dispatch; tm (timing mode 1) gets the marks frame_scale or frame_resize and the two steps' own.
void enqueue_conversion(int fmt, const WriterGeom& g, const uint8_t* src_bgr, int W, int H, const SlotFormat& b, hipStream_t s, hipEvent_t done, Timer* tm);
// the raster step: the I420 kernel into b.i420, the I444 kernel into b.i444 (marks: frame_format), or the PAL8 triple (histogram, build, index plane; marks
// pal8_hist, pal8_build, frame_format) on b.pal8_tables into b.pal8.  Returns the buffer written, which the coder reads; `done` rides on the last dispatch.
const uint8_t* enqueue_raster(FrameRaster raster, const uint8_t* src_bgr, int W, int H, const SlotFormat& b, hipStream_t s, hipEvent_t done, Timer* tm);
// the coder step: `src` (the record's raster form; PNG: the tight BGR frame, any alignment) coded into `frame`, its length also into the pinned word behind
// total_dev (null: none); `done` rides on the last dispatch.  GIF: two dispatches (marks gif_lzw, gif_pack).  JPEG: two (jpeg_code, jpeg_pack), on per-frame tables four (jpeg_count, jpeg_tables in front), in the record's
// sampling at the quality that `tables` (device memory, kernels.h: kJpegTableBytes) name.  PNG: the six of kernels_frame_png.hip (png_filter, png_cost,
// png_scan, png_pack, png_crc, png_finish), under PNG_RUNS with the run-aware cost and pack kernels in the places of the two, under PNG_OPT with the ones that build and use the segments' own tables.
// JPEG under a byte budget (`budget` not empty; POPPY_FRAME_JPEG and POPPY_FRAME_JPEG444 only): kJpegBudgetSteps pairs of dispatches in front (marks jpeg_measure, jpeg_pick),
// then the same two on the picked quality's tables.
void enqueue_coding(const FormatTraits& t, const uint8_t* src, const void* tables, uint8_t* scratch, uint8_t* frame, void* total_dev, int W, int H, hipStream_t s, hipEvent_t done, Timer* tm,
                    const poppy_hip::JpegBudget& budget = poppy_hip::JpegBudget());
hipError_t prepare_coding_scratch(const FormatTraits& t, uint8_t* scratch, int W, int H, hipStream_t s);      // ... once behind its allocation, in front of the first frame coded on it
size_t coding_scratch_bytes(const FormatTraits& t, int W, int H);      // ... and what `scratch` holds (kernels.h: gif_scratch_bytes, jpeg_scratch_bytes, png_scratch_bytes)
// the context's quantisation tables and header for its quality on the device, at an address that stays (captured bodies hold it): allocated and filled when missing
int ensure_jpeg_tables(poppy_hip_ctx* c);
// the byte budget of the context's JPEG frames as the kernels read it: the tables of all 100 qualities and the words (budget, highest quality) behind them, one
// allocation at an address that stays, filled on first use and the words rewritten by the setters once the frames are drained.  *out stays empty with the budget off
// or for a format the budget does not apply to.
int context_jpeg_budget(poppy_hip_ctx* c, const FormatTraits& t, poppy_hip::JpegBudget* out);
int ensure_jpeg_budget_tables(poppy_hip_ctx* c);      // ... the allocation alone (c->jpeg_budget_tables), for a call that brings its own words
// ... and the sequence budget's: the same tables, and the words (JpegSeqBudgetParams: the 64-bit budget, the highest quality) that stand behind the per-frame budget's
// in the same allocation, rewritten by the setters once the frames are drained
int context_jpeg_seq_budget(poppy_hip_ctx* c, poppy_hip::JpegBudget* out);
bool budget_applies(const FormatTraits& t);      // POPPY_FRAME_JPEG and POPPY_FRAME_JPEG444; (the four formats on built tables refuse a budget: poppy_hip_set_frame_format and poppy_hip_set_jpeg_budget, whichever comes second)
// conversion tables, zero before the first frame (the palette builds leave them zero again): PAL8's per slot and for the scratch, the sequence's per context
int alloc_zeroed_tables(poppy_hip_ctx* c, uint8_t** tables, size_t bytes);
