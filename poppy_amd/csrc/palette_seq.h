// palette_seq.h — the sequence formats: one palette (POPPY_FRAME_PAL8_SEQ, POPPY_FRAME_GIF_SEQ), one set of Huffman tables (POPPY_FRAME_JPEG_SEQ,
// POPPY_FRAME_JPEG444_SEQ) or one ninth deflate table (POPPY_FRAME_PNG_SEQ) for all the frames a call hands to its writer.  Owns the context's PaletteSeq — tables, store, the rings of index planes and of coded
// frames — and the two hand-over loops.  palette_seq.cpp.
#pragma once
#include "frame_format.h"
#include "writer_buffers.h"

// seq_begin opens a sequence of n frames (limits, tables, store), every frame for the writer then goes through seq_pass (render_slot, seq_add_image) instead of
// a download, and seq_finish builds the palette (the tables) and hands every frame to the writer; seq_abort ends a sequence of which a frame failed, nothing written.
// The palette sequence's tables (kernels.h: kPal8SeqTableBytes; zero between sequences), the frames held back until the palette is known (`stride` bytes apart, kept
// between sequences, grown when needed), and a ring of index planes on their way to the writer.  The coded sequences (GIF_SEQ, JPEG_SEQ, JPEG444_SEQ): a ring of coded
// frames instead (`coded`: per ring buffer the frame's capacity, then the coder's scratch) and a word of mapped pinned memory per ring buffer that the coder's last
// kernel stores the frame's length into.  The JPEG sequences hold the frames back as the planes of their sampling, not as BGR, and add every frame's symbols into
// `jpeg` (kernels.h: kJpegSeqTableBytes — the sequence's counts, zero between sequences and never cleared between the frames of one, then the tables built from them).
// The PNG sequence holds the frames back as FILTERED STREAMS: a frame's place in the store is a whole PNG_RUNS coder scratch (png_scratch_bytes(w, h, kRunsSeq): the
// stream padded to whole segments, h (1 + 3 w) bytes and under 0.5 % on top at 1080p, 6.2 MB a frame, 374 MB for 60), so that the frame's coder later runs on its
// place and the ring buffers carry no scratch.  The store is kept between sequences and grown when needed, like the others'; it goes with the context.  Every frame's
// tokens are added into `png` (kernels.h: kPngSeqTableBytes — the 286 sums, zero between sequences, then the one table built from them).
// POPPY_FRAME_JPEG and POPPY_FRAME_JPEG444 under a sequence budget (poppy_hip_set_jpeg_sequence_budget; frame_format.h: writer_traits) are held back as the JPEG
// sequences are, as planes, but nothing is counted and no table built: the pass is the raster kernel alone, and seq_finish runs the budget's search ONCE over the
// store — kJpegBudgetSteps steps of one measuring launch over segments x frames and one pick on `budget` — and then codes every frame at the one picked quality
// through the ring of coded frames.  Nothing of it needs clearing between sequences: the first step starts the search from the context's words.
struct PaletteSeq {
    uint8_t* tables = nullptr;
    uint8_t* jpeg = nullptr;
    uint8_t* png = nullptr;
    DeviceBuffer store; size_t stride = 0;
    DeviceBuffer idx, coded;
    DeviceBuffer budget;                  // POPPY_FRAME_JPEG / JPEG444 under a sequence budget: the sequence's one search state, then the lengths its steps measure (kernels.h: jpeg_seq_budget_bytes)
    uint32_t* coded_total = nullptr; uint8_t* coded_total_dev = nullptr;      // kStageRing words, 64 bytes apart
    bool open = false;                    // a sequence is being collected: frames for the writer go through the pass into the store
    int n = 0, count = 0;                 // its frames, and how many of them have been queued
};
int seq_begin(poppy_hip_ctx* c, int n);
bool seq_wanted(const poppy_hip_ctx* c);          // frames submitted now go into the open sequence
uint8_t* seq_next_place(poppy_hip_ctx* c);        // the next frame's place in the store; null: the sequence is full
// the pass of one frame (in the writer's geometry): into the sequence's sums and on to `dst` in the store.  A palette sequence: one kernel.  A JPEG sequence: the
// raster kernel into `dst`, then the counting kernel on it (in timing mode 1 the mark frame_format stands between them).  A PNG sequence: the filter into `dst`,
// then the counting kernel on it (the mark png_filter between them)
int seq_pass(poppy_hip_ctx* c, const uint8_t* d_bgr, uint8_t* dst, hipStream_t s, hipEvent_t done);
const char* seq_pass_mark(const poppy_hip_ctx* c);      // the pass's name in timing mode 1, for the mark behind it: pal8_seq_hist, jpeg_count or png_seq_count
int seq_add_image(poppy_hip_ctx* c, const uint8_t* d_bgr);      // a full-size frame that no slot renders (the t == 0 / 1 copies of poppy_hip_render_phases), on the context's stream
int seq_abort(poppy_hip_ctx* c);
void seq_abort_keep_error(poppy_hip_ctx* c);      // ... behind a failure whose message the caller gets
int seq_finish(poppy_hip_ctx* c, poppy_write_cb write, void* user);      // the open sequence is complete: palette (tables), then every frame to the writer.  Whatever fails in there, the sequence is closed and the tables (the counts) are zero afterwards.
