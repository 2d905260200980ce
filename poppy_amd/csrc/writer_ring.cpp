// writer_ring.cpp — the pinned ring towards the writer (writer_ring.h).
#include "context.h"

int WriterRing::open(poppy_hip_ctx* c, size_t frame_bytes, bool cap_by_slots) {
    static const int ring_pref = getenv("POPPY_HIP_RING") ? std::max(1, atoi(getenv("POPPY_HIP_RING"))) : 3;
    R = std::min(poppy_hip_ctx::kStageRing, ring_pref);
    if (cap_by_slots) R = std::min(R, (int)c->slots.size());
    slot_bytes = (frame_bytes + 255) & ~(size_t)255;
    issued = written = 0;
    if (slot_bytes * R > c->h_stage_bytes) {                      // the context's pinned stage only grows
        if (c->h_stage) (void)hipHostFree(c->h_stage);
        c->h_stage = nullptr; c->h_stage_bytes = 0;
        HIPCHK(c, hipHostMalloc((void**)&c->h_stage, slot_bytes * R, hipHostMallocMapped));
        HIPCHK(c, hipHostGetDevicePointer(&c->h_stage_dev, c->h_stage, 0));
        c->h_stage_bytes = slot_bytes * R;
    }
    base = c->h_stage;
    return POPPY_OK;
}
hipError_t WriterRing::stream(poppy_hip_ctx* c, int k, hipStream_t* s) const {
    hipStream_t& st = c->dl_ring[k % R];
    const hipError_t e = st ? hipSuccess : hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    *s = st;
    return e;
}
hipError_t WriterRing::deliver_next(poppy_hip_ctx* c, bool by_event, uint8_t** frame) {
    const int r = written % R;
    *frame = buffer(written++);
    return by_event ? hipEventSynchronize(c->dl_done[r]) : hipStreamSynchronize(c->dl_ring[r]);
}
