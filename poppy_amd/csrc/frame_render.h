// frame_render.h — one frame on the resident pair: the frame body (pyrdown .. unsharp, with the writer's conversion behind it) and the two halves of a frame,
// PREPARE (plan blob, upload, raster expansion) and RENDER (everything that reads images).  frame_render.cpp.
#pragma once
#include "plan_blob.h"
#include <hip/hip_runtime.h>
#include <vector>

struct poppy_hip_ctx;

// A frame in two halves (round 6).  PREPARE: the slot's plan blob is filled, uploaded and expanded into id bytes + record slots (k_upload, k_tile_expand) — that depends
// on the plan only.  RENDER: everything that reads images.  For chained frames the first half runs on the copy stream and the HOST waits for it before it launches
// the warp kernel (no device-side wait across hardware queues: choose_frame_stream); until round 6 that wait sat between the two halves of the SAME frame — 38 us of every frame's
// ~100 us of host time alone, ~500 us per frame in a pool, where the copy stream's packets queue behind other contexts' kernels.  render_sequence now prepares frame j + 1
// right after it has launched frame j: the wait at the head of frame j + 1 finds the event complete.
// SlotPrep: the frame prepared in a slot (prepare_slot), waiting for its second half (render_slot); one record per slot in poppy_hip_ctx::slot_preps
struct SlotPrep {
    bool valid = false;
    int T = 0, n_work = 0, tile_w = 0;
    bool bin_warp = false, fast_warp = false, chained = false, use_graph = false;
    unsigned long long seq = 0;            // the submit_frame call this was prepared for (0: prepared by that call itself)
    poppy_hip::PlanBlobLayout lay;         // where the frame's groups are in the slot's blob
    double mask = 0;
    hipStream_t s = nullptr;
    std::vector<poppy_hip::P2f> morphed;
};

int submit_frame(poppy_hip_ctx* c, double mask, bool chain);                          // c->plan into the next slot, both halves (the first only if prepare_ahead has not run it)
int prepare_ahead(poppy_hip_ctx* c, const poppy_hip::FramePlan& plan, double mask);   // chained frames: the first half of the frame the NEXT submit_frame renders
void drop_slot_preps(poppy_hip_ctx* c);                                               // no slot holds a prepared frame any more
