// frame_format.h — what depends on the format a writer gets its frames in (poppy_hip_set_frame_format): the formats' facts, a slot's conversion buffers,
// the conversion launches, the POPPY_FRAME_PAL8_SEQ / POPPY_FRAME_GIF_SEQ sequence, the pinned ring towards the writer and the frames that no slot renders.  frame_format.cpp.
#pragma once
#include "../../include/poppy_hip.h"
#include <hip/hip_runtime.h>
#include <vector>

struct poppy_hip_ctx; struct FrameSlot; struct Timer;

bool format_known(int fmt);
const char* format_refuses(int fmt, int W, int H);      // why `fmt` refuses a W x H frame, or null: checked on the arguments alone, before anything is allocated or any state changes
size_t writer_stride(int fmt, int W);      // what the writer is told: 0 for a coded frame (GIF), the width for the planar and palette formats, 3 * width for BGR
// a palette per frame: the PAL8 triple (histogram, build, index plane) converts it — GIF is PAL8 with the two coding dispatches behind the index plane
inline bool format_builds_palette(int fmt) { return fmt == POPPY_FRAME_PAL8 || fmt == POPPY_FRAME_GIF; }
// a frame whose length its bytes decide: poppy_frame_bytes is its capacity, the slot's pinned word holds its length (slot_frame_length)
// (GIF_SEQ: the pinned word is the sequence ring buffer's, seq_finish)
inline bool format_is_coded(int fmt) { return fmt == POPPY_FRAME_GIF || fmt == POPPY_FRAME_GIF_SEQ; }
// one palette for all the frames a call hands to its writer: they wait in the sequence store until the last is rendered (PaletteSeq); GIF_SEQ is PAL8_SEQ coded
inline bool format_is_sequence(int fmt) { return fmt == POPPY_FRAME_PAL8_SEQ || fmt == POPPY_FRAME_GIF_SEQ; }
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
bool size_admits(int W, int H, int ow, int oh);      // the rule's admissible sizes (include/poppy_hip.h)
WriterGeom context_geom(const poppy_hip_ctx* c, int W, int H, bool has_writer = true);      // of a W x H frame under the context's scale or size (which W x H admits: writer_refuses)
WriterGeom writer_geom(const poppy_hip_ctx* c, bool has_writer = true);      // of the resident pair's frames
const char* writer_refuses(const poppy_hip_ctx* c, int fmt, int W, int H);      // why a W x H frame cannot go to a writer under the context's scale or size in format `fmt`, or null: the size's admission, then format_refuses on the writer's geometry
void launch_writer_scaling(const WriterGeom& g, const uint8_t* src, uint8_t* dst, int W, int H, hipStream_t s, hipEvent_t done = nullptr);      // W x H -> g on the device (g.scaled()): the whole-factor downscale or the area resize
const char* scaling_mark(const WriterGeom& g);      // its name in timing mode 1: frame_scale or frame_resize
int writer_format(const poppy_hip_ctx* c, bool has_writer);      // the format of the frames a call hands to its writer (none: they stay BGR in HBM), and whether they are collected into one palette sequence first
bool writer_wants_sequence(const poppy_hip_ctx* c, bool has_writer);

struct SlotFormat {
    uint8_t* scaled = nullptr;            // a scale above 1 or a size: the frame scaled down, tight BGR, ow x oh — what the conversion reads and, under BGR, what the writer gets
    uint8_t* i420 = nullptr;              // the frame as I420 for the writer (allocated when the format is I420 and a pair is there; kept until the pair's buffers go)
    uint8_t* pal8 = nullptr;              // the frame as PAL8 for the writer, and the conversion's tables (kernels.h: kPal8TableBytes) — the slot's own,
    uint8_t* pal8_tables = nullptr;       // because the conversions of frames in flight run beside each other (allocated like i420; the stream and event live as long as the context)
    uint8_t* gif = nullptr;               // POPPY_FRAME_GIF: the coded frame for the writer (its capacity: poppy_frame_bytes), the coder's scratch (kernels.h: gif_scratch_bytes)
    uint8_t* gif_scratch = nullptr;       // ... and a word of mapped pinned memory that k_gif_pack stores the frame's length into: the host reads it when `done`
    uint32_t* gif_total = nullptr;        // has fired and copies that many bytes (the PAL8 frame the coder reads is the slot's pal8)
    void* gif_total_dev = nullptr;
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

// src_bgr (W x H) scaled down to g into b.scaled (g.scaled(): the first dispatch) and in format `fmt` into b's buffers on stream s: the I420 kernel, or the PAL8
// triple and, for GIF, the coding pair behind it.  `done` (optional) rides on the last dispatch; tm (timing mode 1) gets the marks frame_scale or frame_resize,
// frame_format, pal8_hist, pal8_build, gif_lzw, gif_pack.
void enqueue_conversion(int fmt, const WriterGeom& g, const uint8_t* src_bgr, int W, int H, const SlotFormat& b, hipStream_t s, hipEvent_t done, Timer* tm);

// POPPY_FRAME_PAL8_SEQ and POPPY_FRAME_GIF_SEQ: one palette for all the frames a call hands to its writer.
// seq_begin opens a sequence of n frames (limits, tables, store), every frame for the writer then goes through seq_pass (render_slot, seq_add_image) instead of
// a download, and seq_finish builds the palette and hands every frame to the writer; seq_abort ends a sequence of which a frame failed, nothing written.
// The sequence's tables (kernels.h: kPal8SeqTableBytes; zero between sequences), the frames held back until the palette is known (`stride` bytes apart, kept between
// sequences, grown when needed), and a ring of index planes on their way to the writer.  GIF_SEQ: a ring of coded frames instead (`gif`: per ring buffer the frame's
// capacity, then the coder's scratch, `gif_each` bytes apart) and a word of mapped pinned memory per ring buffer that k_gif_pack stores the frame's length into.
struct PaletteSeq {
    uint8_t* tables = nullptr;
    uint8_t* store = nullptr; size_t store_bytes = 0, stride = 0;
    uint8_t* idx = nullptr; size_t idx_bytes = 0;
    uint8_t* gif = nullptr; size_t gif_bytes = 0;
    uint32_t* gif_total = nullptr; uint8_t* gif_total_dev = nullptr;      // kStageRing words, 64 bytes apart
    bool open = false;                    // a sequence is being collected: frames for the writer go through the pass into the store
    int n = 0, count = 0;                 // its frames, and how many of them have been queued
};
int seq_begin(poppy_hip_ctx* c, int n);
bool seq_wanted(const poppy_hip_ctx* c);          // frames submitted now go into the open sequence
uint8_t* seq_next_place(poppy_hip_ctx* c);        // the next frame's place in the store; null: the sequence is full
int seq_pass(poppy_hip_ctx* c, const uint8_t* d_bgr, uint8_t* dst, hipStream_t s, hipEvent_t done);      // the pass of one frame (in the writer's geometry): into the sequence's sums and on to `dst` in the store, one kernel
int seq_add_image(poppy_hip_ctx* c, const uint8_t* d_bgr);      // a full-size frame that no slot renders (the t == 0 / 1 copies of poppy_hip_render_phases), on the context's stream
int seq_abort(poppy_hip_ctx* c);
void seq_abort_keep_error(poppy_hip_ctx* c);      // ... behind a failure whose message the caller gets
int seq_finish(poppy_hip_ctx* c, poppy_write_cb write, void* user);      // the open sequence is complete: palette, then every frame to the writer.  Whatever fails in there, the sequence is closed and the tables are zero afterwards.

// R pinned buffers, frame k in buffer k mod R: the copy of frame `issued` is the next to be queued, frame `written` the next the writer gets.
struct WriterRing {
    int R = 1;
    size_t slot_bytes = 0;                // ring slots start on 256-byte boundaries
    int issued = 0, written = 0;
    uint8_t* base = nullptr;
    int open(poppy_hip_ctx* c, size_t frame_bytes, bool cap_by_slots);      // POPPY_HIP_RING buffers (default 3; at most kStageRing and, where the frames come from the slots, the slot count) of frame_bytes in the context's pinned stage
    uint8_t* buffer(int k) const { return base + (size_t)(k % R) * slot_bytes; }
    hipError_t stream(poppy_hip_ctx* c, int k, hipStream_t* s) const;      // the stream of frame k's buffer, which carries nothing but that buffer's copies (created at first use)
    hipError_t deliver_next(poppy_hip_ctx* c, bool by_event, uint8_t** frame);      // waits for the copy of frame `written` — its buffer's stream, or with by_event the ring event recorded behind it — and counts it as handed over
};

// a device frame (tight u8x3, W x H) in the writer's geometry g = context_geom(c, W, H) and format in `host`, queued on c->stream and waited for;
// *stride = what the writer is told
// n_copies: how often the writer gets this frame — under the sequence formats these copies are the whole sequence, and the frame is converted on the host
int download_frame(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, const WriterGeom& g, std::vector<uint8_t>& host, size_t* stride, int n_copies = 1);
const uint8_t* host_frame(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, std::vector<uint8_t>& tmp, size_t* out_stride, int* status, int n_copies = 1);      // a host frame (already in the writer's geometry) in the writer's format: `bgr` itself (BGR) or its I420 / PAL8 / coded form in `tmp`; nullptr, *status and c->err set, when the format refuses the frame
int write_device_image(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, int n_copies, poppy_write_cb write, void* user);      // a device image / a host image to the writer, n_copies times, in the writer's format (the phase 0 / 1 and t = 0 / 1 copies, the linear-blend fallback frames)
int write_host_image(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, int n_copies, poppy_write_cb write, void* user);
int pal8_seq_of_copies(const uint8_t* bgr, size_t stride, int n_copies, int width, int height, uint8_t* dst);      // frame_pal8.cpp: the POPPY_FRAME_PAL8_SEQ frame of a sequence that is n_copies times the same BGR frame (poppy_bgr_frames_to_pal8 with frame_stride 0, one frame out)
