// frame_sequence.h — the multi-frame driver: the plans of a sequence made by the context's planner team (possibly ahead of the call that takes them), the
// single frame and the sequence of frames on the resident pair, with the download pump towards a writer.  frame_sequence.cpp.
#pragma once
#include "../../include/poppy_hip.h"
#include "frame_plan.h"
#include <atomic>
#include <vector>

struct poppy_hip_ctx;

// The plans of one multi-frame call, made by the context's planner team.  They live on the heap because the team may be started BEFORE the call that consumes them
// (round 6): a pair loader starts the plans of the reference's default sequence — number_of_frames chained frames, src/poppy.hpp:177-210 — the moment the point pairs are
// known, while the set-up's last kernels and copies still run; poppy_hip_morph_frames then finds its first plans ready instead of idling the GPU for the 0.3-0.5 ms the
// first plan takes (one context, pair after pair: 4 % of a pair).  A call with other frames drops them (the planners stop at their next frame) and makes its own.
struct SeqPlans {
    int n = 0, W = 0, H = 0;
    bool chain = false, abandoned = false;                     // abandoned: told to stop before every frame was planned (never adopted)
    std::vector<double> shape;
    std::vector<poppy_hip::P2f> pts1_at_start, pts2;           // the point sets the plans were made from (a call adopts them only for the same ones)
    std::vector<std::vector<poppy_hip::P2f>> src1;
    std::vector<poppy_hip::FramePlan> plans;
    std::vector<int> rcs;
    std::vector<std::atomic<int>> ready;
    std::atomic<int> next{0};
    explicit SeqPlans(int n_) : n(n_), src1(n_), plans(n_), rcs(n_, 0), ready(n_) { for (auto& r : ready) r.store(0); }
};

extern std::atomic<int> g_live_contexts;        // contexts alive in this process: they share the host's threads for their frame planners
void start_default_seq_plans(poppy_hip_ctx* c);                // a pair loader's speculative start (set_points): the reference's default sequence on the new pair
// The one end of a context's SeqPlans: tells the planners to stop at their next frame, waits for the team and releases the plans.
// false: a planner thread threw (c->planners.error()).
bool end_seq_plans(poppy_hip_ctx* c);

int render_frame(poppy_hip_ctx* c, double shape, double mask, bool chain);            // one frame on the resident pair; result in the slot c->last_slot
int render_sequence(poppy_hip_ctx* c, const double* shape, const double* mask, int n, bool chain, poppy_write_cb write, void* user, bool in_open_seq = false);
