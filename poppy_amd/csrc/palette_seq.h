// palette_seq.h — POPPY_FRAME_PAL8_SEQ and POPPY_FRAME_GIF_SEQ: one palette for all the frames a call hands to its writer.  Owns the context's PaletteSeq — tables,
// store, the rings of index planes and of coded frames — and the two hand-over loops.  palette_seq.cpp.
#pragma once
#include "frame_format.h"
#include "writer_buffers.h"

// seq_begin opens a sequence of n frames (limits, tables, store), every frame for the writer then goes through seq_pass (render_slot, seq_add_image) instead of
// a download, and seq_finish builds the palette and hands every frame to the writer; seq_abort ends a sequence of which a frame failed, nothing written.
// The sequence's tables (kernels.h: kPal8SeqTableBytes; zero between sequences), the frames held back until the palette is known (`stride` bytes apart, kept between
// sequences, grown when needed), and a ring of index planes on their way to the writer.  GIF_SEQ: a ring of coded frames instead (`gif`: per ring buffer the frame's
// capacity, then the coder's scratch, `gif_each` bytes apart) and a word of mapped pinned memory per ring buffer that k_gif_pack stores the frame's length into.
struct PaletteSeq {
    uint8_t* tables = nullptr;
    DeviceBuffer store; size_t stride = 0;
    DeviceBuffer idx, gif;
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
