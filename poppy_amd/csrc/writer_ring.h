// writer_ring.h — the pinned ring towards the writer, in the context's pinned stage (which only grows): frame_sequence.cpp's FramePump and the two sequence
// hand-overs (palette_seq.cpp) queue their copies through it.  writer_ring.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

struct poppy_hip_ctx;

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
