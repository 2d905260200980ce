// frame_render.cpp — one frame on the resident pair (frame_render.h): the frame body, pyrdown .. unsharp with the writer's conversion behind it, and the two
// halves of a frame, prepare_slot (plan blob, upload, raster expansion) and render_slot (everything that reads images).  Which frames are rendered, and what
// becomes of them, is frame_sequence.cpp's.
#include "context.h"
#include <chrono>

static_assert(kPlanRasterRows == kRasterChunkRows, "the plan's work list and k_raster must agree on the chunk height");

// the format the frames being submitted are converted to for their writer (their slots' bodies end with the conversion); BGR: none
// (PAL8_SEQ, GIF_SEQ: none either — the sequence pass is launched behind the body, its destination differs from frame to frame: render_slot)
static int frame_wants_format(const poppy_hip_ctx* c) { return c->writer_attached && !writer_traits(c, c->frame_format).sequence ? c->frame_format : POPPY_FRAME_BGR; }
// ... and the geometry they are scaled down or resized to in front of it, under every format (the sequence formats' pass reads the scaled frame)
// ... and whether its conversion runs the JPEG byte budget's search (what enqueue_conversion reads: the slot's budget, under a format that applies it)
static bool frame_wants_budget(const poppy_hip_ctx* c, const FrameSlot& f) { return budget_applies(*format_traits(frame_wants_format(c))) && (bool)f.fmt.jpeg_budget; }
static WriterGeom frame_wants_geom(const poppy_hip_ctx* c) { return writer_geom(c, c->writer_attached); }

// pyrdown .. unsharp of one slot.  Every argument is fixed for the life of the pair (the per-frame unsharp amount is
// read from the slot's plan blob), which is what lets the whole sequence be captured into one graph launch.
static int enqueue_body(poppy_hip_ctx* c, FrameSlot& f, hipStream_t s, Timer* tm, float amount, bool debug, hipEvent_t done = nullptr, bool chained = false,
                        uint8_t* seq_dst = nullptr) {
    const int W = c->W, H = c->H, L = c->cfg.pyramid_levels;
    const int ft = c->first_tail < L ? c->first_tail : L;
    static const bool fuse = getenv("POPPY_HIP_NOFUSE") == nullptr;
    // debug frames only (issued by the calling thread, never captured): the launch list for poppy_hip_last_pyramid_forms
    if (debug) c->pyr_forms.clear();
    auto rec = [&](int kind, int level, int arg) { if (debug) c->pyr_forms.insert(c->pyr_forms.end(), {kind, level, arg}); };
    for (int i = 0; i < ft;) {
        const PyrLevel &a = c->levels[i], &b = c->levels[i + 1];
        if (fuse && i >= 1 && i + 2 <= ft && b.pitch == b.w && c->levels[i + 2].pitch == c->levels[i + 2].w && pyrdown2_eligible(a.w, a.h)) {     // two small levels in one launch (the two it writes are tight)
            const PyrLevel& d = c->levels[i + 2];
            launch_pyrdown2(f.pyrL + a.off3, f.pyrR + a.off3, f.pyrM + a.off1, f.pyrL + b.off3, f.pyrR + b.off3, f.pyrM + b.off1,
                            f.pyrL + d.off3, f.pyrR + d.off3, f.pyrM + d.off1, a.w, a.h, s, a.pitch);
            rec(POPPY_PYR_DOWN2, i, 0);
            i += 2;
            continue;
        }
        const void* sl = i == 0 ? (const void*)f.tr1 : (const void*)(f.pyrL + a.off3);
        const void* sr = i == 0 ? (const void*)f.tr2 : (const void*)(f.pyrR + a.off3);
        const bool lazy = i == 0 && c->lazy_mask;      // level 0 reads the mask through m2 (kernels.h: launch_pyrdown)
        launch_pyrdown(sl, sr, lazy ? c->m2 : f.pyrM + a.off1, i == 0, f.pyrL + b.off3, f.pyrR + b.off3, f.pyrM + b.off1, a.w, a.h, s,
                       lazy ? (const double*)(f.d_blob + kBlobMaskAB) : nullptr, a.pitch, lazy ? a.w : a.pitch, b.pitch);
        rec(POPPY_PYR_DOWN, i, lazy);
        ++i;
    }
    if (tm) tm->mark("pyrdown");
    if (c->use_tail) launch_pyr_tail(f.pyrL, f.pyrR, f.pyrM, f.pyrB, c->d_levels, c->tail.args, c->tail.lds_bytes, s);
    else launch_mix_top(f.pyrL + c->levels[L].off3, f.pyrR + c->levels[L].off3, f.pyrM + c->levels[L].off1, f.pyrB + c->levels[L].off3,
                        c->levels[L].pitch * c->levels[L].h, s);      // element-wise: a padded level's rows are mixed with their padding
    if (c->use_tail) { rec(POPPY_PYR_TAIL, ft, c->tail.args.n_wide); rec(POPPY_PYR_TAIL_NL, L, c->tail.args.nl); }
    else rec(POPPY_PYR_MIX_TOP, L, 0);
    if (tm) tm->mark("pyr_tail");
    // The way up: the small levels in ONE launch (round 6, kernels_pyramid_cone.hip): from the tail's level to the largest level of at most kConeMaxPixels
    // (level 1 at 1080p, level 2 at 4K).  POPPY_HIP_NOCONE: the launches of round 5 (k_collapse2 pairs + one k_collapse_level per remaining level).
    static const bool cone = getenv("POPPY_HIP_NOCONE") == nullptr;
    int j_top = ft;
    if (fuse && cone) {
        int k = 1;
        while (k < ft && (size_t)c->levels[k].w * c->levels[k].h > kConeMaxPixels) ++k;
        if (ft - k > kConeMaxLevels) k = ft - kConeMaxLevels;
        if (ft - k >= 2 && collapse_cone_eligible(&c->levels[k], ft - k)) {
            launch_collapse_cone(f.pyrL, f.pyrR, f.pyrM, f.pyrB, &c->levels[k], ft - k, s);
            rec(POPPY_PYR_CONE, k, ft - k);
            j_top = k;
        }
    }
    for (int j = j_top; j > 0;) {                  // blended level j is known; produce level j-2 or j-1
        if (fuse && j - 2 >= 1) {
            const PyrLevel &a = c->levels[j - 2], &m = c->levels[j - 1], &n = c->levels[j];
            if (a.pitch == a.w && m.pitch == m.w && collapse2_eligible(a.w, a.h, m.w, m.h, n.w, n.h)) {
                launch_collapse2(f.pyrL + a.off3, f.pyrR + a.off3, f.pyrM + a.off1, f.pyrL + m.off3, f.pyrR + m.off3, f.pyrM + m.off1,
                                 f.pyrL + n.off3, f.pyrR + n.off3, f.pyrB + n.off3, f.pyrB + a.off3, a.w, a.h, m.w, m.h, n.w, n.h, s);
                rec(POPPY_PYR_UP2, j - 2, 0);
                j -= 2;
                continue;
            }
        }
        const int i = j - 1;
        const PyrLevel &a = c->levels[i], &b = c->levels[i + 1];
        const void* gl = i == 0 ? (const void*)f.tr1 : (const void*)(f.pyrL + a.off3);
        const void* gr = i == 0 ? (const void*)f.tr2 : (const void*)(f.pyrR + a.off3);
        const bool lazy = i == 0 && c->lazy_mask;
        launch_collapse(gl, gr, i == 0, lazy ? c->m2 : f.pyrM + a.off1, f.pyrL + b.off3, f.pyrR + b.off3, f.pyrB + b.off3, f.pyrB + a.off3,
                        a.w, a.h, b.w, b.h, s, lazy ? (const double*)(f.d_blob + kBlobMaskAB) : nullptr, a.pitch, lazy ? a.w : a.pitch, b.pitch);
        rec(POPPY_PYR_UP, i, lazy);
        --j;
    }
    if (tm) tm->mark("collapse");
    // A frame for a writer that takes I420 is converted right behind its unsharp, on the same stream, and the frame's completion event rides on the
    // conversion: the host waits for that event, then issues the copy of the slot's I420 buffer (render_sequence_frames), which depends on nothing.
    // PAL8 is three dispatches, and the palette build in the middle is one workgroup's serial work (about as long as the rest of the frame).  The next chained
    // frame needs this frame's BGR, not its palette form: on the chain (`chained` with a completion event riding, i.e. kernels launched one by one) the
    // conversion goes to the slot's side stream behind an event that rides on the unsharp, the chain's stream goes on with the next frame, and `done` —
    // which the download, the slot's reuse and drain_frames wait for — rides on the conversion's last dispatch (frame_format.cpp: enqueue_conversion).
    // GIF is PAL8 with the two coding dispatches behind the index plane, wherever PAL8's run; `done` rides on the second.
    // JPEG is I420 with its two coding dispatches behind the conversion, wherever I420's runs: on the chain's own stream.  Nothing in them is one workgroup's
    // serial work — a wave per restart interval, a thousand of them at 1080p, 46 us in all —, and on the slot's low-priority side stream they were measured
    // slower, not faster: the chained 1080p frame 4.5 - 4.8k frames/s against 5.5k here, a pool of six 4.5 - 4.7k against 6.8 - 6.9k.
    // PNG (and PNG_RUNS, PNG_OPT) is six dispatches straight behind the unsharp, on the chain's own stream as JPEG's: the two that are one workgroup's work (scan, finish) are short.
    // PAL8_SEQ (seq_dst: the frame's place in the sequence store, never set in a captured body): the pass takes PAL8's place, on the side stream too — it is short,
    // but the chain needs nothing of it.
    // JPEG_SEQ and JPEG444_SEQ: the pass is the raster kernel into the store and the counting kernel on it, 27 - 38 us at 1080p and nothing of it one workgroup's serial
    // work, so it stays on the chain's own stream as JPEG's coder does.  On the side stream it was measured at 2.8k chained frames/s against 5.0k here: `done` rides on the
    // pass, the low-priority queue runs it late, and the slot's reuse waits for it ("JPEG sequence-table hand-off").
    // PNG_SEQ: the pass is PNG's filter into the frame's place in the store and the counting kernel on it, a workgroup per row and per segment and nothing serial, so
    // it stays on the chain's own stream for JPEG_SEQ's reason; everything else of the coder runs behind the sequence's build, in the hand-over loop.
    // A scale above 1 or a size: the downscale (the resize) is the conversion's first dispatch wherever that runs, and a conversion of its own under BGR (the writer gets the slot's
    // scaled frame); the chain goes on from the full-size frame.
    const int fmt = frame_wants_format(c);
    const WriterGeom geom = frame_wants_geom(c);
    const FormatTraits& traits = *format_traits(fmt);
    const bool side = (traits.slot_raster() == kRasterPal8 || (seq_dst && traits.raster == kRasterPal8)) && chained && done && !tm;
    const bool converts = traits.converts() || seq_dst || geom.scaled();
    launch_unsharp(f.pyrB, f.tmp, f.diff, f.out, debug ? f.unsharpF : nullptr, W, H, amount, (const float*)f.d_blob, (float)0.3, s,
                   side ? f.fmt.bgr_done : converts ? nullptr : done, c->levels[0].pitch);
    rec(POPPY_PYR_UNSHARP, 0, W < 2 || H < 2);
    if (tm) tm->mark("unsharp");
    if (!converts) return POPPY_OK;
    hipStream_t fs = side ? f.fmt.fmt_stream : s;
    if (side) HIPCHK(c, hipStreamWaitEvent(fs, f.fmt.bgr_done, 0));
    if (!seq_dst) { enqueue_conversion(fmt, geom, f.out, W, H, f.fmt, fs, done, tm); return POPPY_OK; }
    if (geom.scaled()) enqueue_conversion(POPPY_FRAME_BGR, geom, f.out, W, H, f.fmt, fs, nullptr, tm);
    { int rc = seq_pass(c, slot_bgr(f, geom), seq_dst, fs, done); if (rc) return rc; }
    if (tm) tm->mark(seq_pass_mark(c));
    return POPPY_OK;
}

static int capture_body(poppy_hip_ctx* c, FrameSlot& f) {
    hipGraph_t g = nullptr;
    HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    (void)enqueue_body(c, f, c->stream, nullptr, 0.f, false);
    f.body_format = frame_wants_format(c); f.body_geom = frame_wants_geom(c); f.body_budget = frame_wants_budget(c, f);
    HIPCHK(c, hipStreamEndCapture(c->stream, &g));
    hipError_t e = hipGraphInstantiate(&f.body, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) { f.body = nullptr; c->err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

void drop_slot_preps(poppy_hip_ctx* c) { for (SlotPrep& p : c->slot_preps) p.valid = false; }

// the slot the next frame renders into: the next one in the ring that does not hold the image that frame reads as corrected1
static int pick_slot(const poppy_hip_ctx* c) {
    int fi = c->next_slot;
    if (c->slots[fi].out == c->cur1) fi = (fi + 1) % (int)c->slots.size();
    return fi;
}

// host waits for an event / for a stream, accounted in `acc` (c->wait_ms: POPPY_SEQ_TIMING)
static hipError_t timed_event_wait(double& acc, hipEvent_t ev) {
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = hipEventSynchronize(ev);
    acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return e;
}
static hipError_t timed_stream_wait(double& acc, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = hipStreamSynchronize(s);
    acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return e;
}

// the device addresses of the groups of the plan in slot f's blob (plan_blob.h; a group the frame did not upload has offset 0 and is not read)
struct BlobPtrs {
    const float* rec; const RasterTri* edges; const OutlineSeg* outl; const int* toff; const uint16_t* ttri;
    const int* tri; const float* inv; const int* work;
};
static BlobPtrs blob_ptrs(const FrameSlot& f, const PlanBlobLayout& l) {
    const uint8_t* d = f.d_blob;
    return {(const float*)(d + kBlobHeader), (const RasterTri*)(d + l.o_edges), (const OutlineSeg*)(d + l.o_outl), (const int*)(d + l.o_toff),
            (const uint16_t*)(d + l.o_ttri), (const int*)(d + l.o_tri), (const float*)(d + l.o_inv), (const int*)(d + l.o_work)};
}

// Streams.  Device-side waits between streams that sit on different hardware queues cost 12-20 us each on this part
// (profiles/r01_e_streams.md), and which streams share a queue is the runtime's choice (GPU_MAX_HW_QUEUES); phase-mode frames
// ran at 8.3k or at 5.2k frames/s depending on it (tools/experiments/frames_only.py).  So no frame waits on another stream's
// event on the device:
//   chained frames      every kernel on the context's stream; the plan upload and the raster expansion run on the copy stream
//                       beside the previous frame and the HOST waits for them (it is a frame ahead of the GPU anyway);
//   independent frames  everything — upload, expansion, kernels — in order on the slot's own stream; the other slots' frames
//                       hide the upload.  Whoever needs all frames finished drains the slot streams (drain_frames).
static int choose_frame_stream(poppy_hip_ctx* c, FrameSlot& f, int fi, bool chained, hipStream_t* out) {
    if (!chained) {
        // Independent frames: a stream per slot (created on first use) when the frames stay in HBM — four frames in flight, 10.7k frames/s at 1080p.
        // With a writer attached the slots take the context's OWN three compute streams in turn — rendering, plan upload, the set-up's second —:
        // a hardware queue is in order, the runtime spreads streams over four of them as they are created, and a fifth stream lands on the queue
        // of the download stream, whose packets wait for every frame copy in front of that slot's kernels (one slot in four behind the copies:
        // a 480-frame sequence with a writer took 80 ms; 74 with the slots on the three queues that carry no copies; without a writer three
        // queues are slower than four, 8.7k frames/s).  POPPY_PHASE_OWN_STREAMS: a stream per slot in both cases, as before round 3.
        static const bool own_streams = getenv("POPPY_PHASE_OWN_STREAMS") != nullptr;
        if (c->writer_attached && !own_streams) {
            if (!c->aux_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
            hipStream_t pick[3] = {c->stream, c->copy_stream, c->aux_stream};
            f.stream = pick[fi % 3];
        } else {
            if (!f.own_stream) HIPCHK(c, hipStreamCreateWithFlags(&f.own_stream, hipStreamNonBlocking));
            f.stream = f.own_stream;
        }
    }
    hipStream_t s = chained ? c->stream : f.stream;
    if (f.last_stream && f.last_stream != s) HIPCHK(c, hipEventSynchronize(f.done));     // the mode changed: settle the slot's last frame once, on the host
    f.last_stream = s;
    *out = s;
    return POPPY_OK;
}

// first half: `plan` into slot fi (blob, upload, expansion).  chained: on the copy stream, nobody waits here.
static int prepare_slot(poppy_hip_ctx* c, const FramePlan& plan, double mask, bool chain, int fi) {
    const int W = c->W, H = c->H;
    const int T = plan.n_tris;
    if (T > c->max_tris) return fail(c, POPPY_E_ARG, "triangle budget exceeded");
    static_assert(((long long)kIdTagMax << kIdTagShift) + (1ll << kIdTagShift) - 1 <= 0x7fffffffll, "tagged ids must stay positive int32 values");
    if (T + 1 >= (1 << kIdTagShift)) return fail(c, POPPY_E_UNSUPPORTED, "more triangles than the id map's tag scheme can number (2^20 - 2)");
    FrameSlot& f = c->slots[fi];
    SlotPrep& pr = c->slot_preps[fi];
    pr.valid = false;
    HIPCHK(c, timed_event_wait(c->wait_ms[1], f.uploaded));        // the pinned copy is free again
    const double amount = std::sin(mask * M_PI);
    *(float*)f.h_blob = (float)(1.0 - amount);                     // unsharp_mask(.., 1, 1.0 - amount, 0.3)
    ((double*)(f.h_blob + kBlobMaskAB))[0] = 1.0 - mask;           // lbmask = clamp(alpha + m2 * beta), read by the level-0 blend kernels
    ((double*)(f.h_blob + kBlobMaskAB))[1] = -mask;
    const int n_work = (int)(plan.work.size() / 2);
    const size_t n_toff = plan.tile_off.size(), n_ttri = plan.tile_tris.size();
    static const bool idmap_only = getenv("POPPY_HIP_IDMAP") != nullptr;
    const bool bins = plan.bins_ok && !idmap_only && !c->debug && n_ttri <= c->bins_cap && plan.max_tile_entries <= warp_bin_max_tile_entries() &&
                      plan.tile_w == warp_bin_tile_width(W, H);
    // the fast warp kernels take the frame when every matrix passes the host's range check (always, short of degenerate input)
    static const bool exact_warp_only = getenv("POPPY_HIP_GENERALWARP") != nullptr;
    // the slot's plan blob (plan_blob.h): the records end at the same place on both paths, and pack_warp_records writes them before the path is known
    const PlanBlobLayout idmap_lay = plan_blob_layout(T, (size_t)n_work, n_toff, n_ttri, false);
    if (idmap_lay.o_edges > c->blob_bytes) return fail(c, POPPY_E_ARG, "plan blob overflow");
    const bool records_ok = pack_warp_records(plan.inv1.data(), plan.inv2.data(), T, W, H, (float*)(f.h_blob + kBlobHeader), plan.tri_xy.data()) && !exact_warp_only;
    // raster fused into the warp kernel: no id map at all.  Any width whose level-0 rows begin on 16-byte boundaries: multiples of 4, and every width from
    // 150 001 pixels up (level_pitch); small images of other widths keep the id-map path
    const bool bin_warp = records_ok && bins && warp_bin_geometry(W, H) && (c->levels[0].pitch & 3) == 0;
    const bool fast_warp = bin_warp || (records_ok && warp_fast_geometry(W, H));
    const PlanBlobLayout lay = bin_warp ? plan_blob_layout(T, (size_t)n_work, n_toff, n_ttri, true) : idmap_lay;
    if (lay.used > c->blob_bytes) return fail(c, POPPY_E_ARG, "plan blob overflow");
    fill_plan_blob(f.h_blob, lay, plan, bin_warp);
    const BlobPtrs d = blob_ptrs(f, lay);

    static const bool no_graph = getenv("POPPY_HIP_NOGRAPH") != nullptr;
    const bool chained = chain || c->cur1_ready;
    hipStream_t s = nullptr;
    { int rc = choose_frame_stream(c, f, fi, chained, &s); if (rc) return rc; }
    if (c->debug && !f.unsharpF) HIPCHK(c, hipMalloc((void**)&f.unsharpF, (size_t)W * H * 12));
    const bool all_marks = c->timing == 1;
    // The captured body is for frames in flight beside each other (phase mode), where the submitting host thread is the
    // bottleneck.  On the chained critical path a graph launch leaves the GPU idle ~8 us longer than the same kernels
    // launched one by one (4600 vs 4785 frames/s, profiles/r01_e_streams.md), and the host keeps up easily.
    const bool use_graph = !no_graph && !chained && !c->debug && !all_marks && W > 1 && H > 1;
    if (use_graph && f.body && (f.body_format != frame_wants_format(c) || f.body_geom != frame_wants_geom(c) || f.body_budget != frame_wants_budget(c, f))) {      // the body has (not) the downscale, the conversion and the budget's search the frame needs: captured again
        HIPCHK(c, hipEventSynchronize(f.done));                                // (the slot's last frame may still run it)
        (void)hipGraphExecDestroy(f.body); f.body = nullptr;
    }
    if (use_graph && !f.body) { int rc = capture_body(c, f); if (rc) return rc; }

    pr.T = T; pr.n_work = n_work; pr.tile_w = plan.tile_w; pr.bin_warp = bin_warp; pr.fast_warp = fast_warp; pr.chained = chained; pr.use_graph = use_graph;
    pr.lay = lay; pr.mask = mask; pr.s = s; pr.morphed = plan.morphed; pr.seq = c->frame_seq;
    hipStream_t up = chained ? c->copy_stream : s;
    if (chained) HIPCHK(c, timed_event_wait(c->wait_ms[2], f.done));       // the frame that last read this slot's device copy of the plan (2+ frames back)
    launch_upload(f.h_blob_dev, f.d_blob, lay.used, up);
    // the raster of the frame, as one id byte per pixel + the tiles' record slots: needs the plan only
    if (bin_warp) launch_tile_expand(d.rec, d.edges, d.outl, d.toff, d.ttri, f.tile_data, plan.tile_w, W, H, up);
    // (The blend mask also depends on the plan only.  Taking it out of the warp kernel — a kernel of its own on this stream —
    // made that kernel faster (20.5 -> 18.1 us at 1080p, 53.6 -> 46.5 us at 4K) and the chained FRAME slower (183.8 -> 188.3 us,
    // 403 -> 411 us): the extra traffic beside the chain costs the chain's bandwidth-bound kernels more than the rider did.
    // profiles/r02_notes.md.)
    HIPCHK(c, hipEventRecord(f.uploaded, up));
    pr.valid = true;
    return POPPY_OK;
}

// the warp of the frame prepared in slot f — fused raster + warp, tiled (id map + records) or general (id map + matrices) —, with the dispatch's stamps when given
static void launch_frame_warp(poppy_hip_ctx* c, FrameSlot& f, const SlotPrep& pr, const BlobPtrs& d, const WarpExtras& ex, hipStream_t s,
                              hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr) {
    const int W = c->W, H = c->H;
    if (pr.bin_warp) launch_warp_bin(d.rec, f.tile_data, c->tile_bytes, d.toff, pr.tile_w, c->cur1, c->c2, f.tr1, f.tr2, W, H, ex, s, t0, t1);
    else if (pr.fast_warp) launch_warp_fast(f.triMap, d.rec, pr.T + 1, c->cur1, c->c2, f.tr1, f.tr2, W, H, ex, s, t0, t1);
    else launch_warp(f.triMap, d.inv, d.inv + (size_t)pr.T * 9, c->cur1, c->c2, f.tr1, f.tr2, W, H, ex, s, t0, t1);
}

// second half: the frame prepared in slot fi
static int render_slot(poppy_hip_ctx* c, int fi, bool chain) {
    const int W = c->W, H = c->H;
    FrameSlot& f = c->slots[fi];
    SlotPrep& pr = c->slot_preps[fi];
    if (!pr.valid) return fail(c, POPPY_E_STATE, "frame slot not prepared");
    pr.valid = false;
    const bool bin_warp = pr.bin_warp, fast_warp = pr.fast_warp, chained = pr.chained, use_graph = pr.use_graph;
    const double mask = pr.mask, amount = std::sin(mask * M_PI);
    hipStream_t s = pr.s;
    const BlobPtrs d = blob_ptrs(f, pr.lay);
    c->last_warp_fast = fast_warp; c->last_warp_bin = bin_warp;
    ++(bin_warp ? c->n_warp_bin : fast_warp ? c->n_warp_fast : c->n_warp_general);
    // a frame of this slot may still be on its way to the writer (the ring only orders the HOST side): nothing may render into
    // `out` before that copy has read it
    if (f.dl_pending) {
        // (unless POPPY_HIP_DL_EVENTS is set: the copy's own stream instead of an event)
        if (f.dl_ring_idx >= 0) HIPCHK(c, timed_stream_wait(c->wait_ms[0], c->dl_ring[f.dl_ring_idx]));
        else HIPCHK(c, timed_event_wait(c->wait_ms[0], f.downloaded));
        f.dl_pending = false;
    }
    const bool all_marks = c->timing == 1;
    Timer tm(c, s);
    if (all_marks) tm.mark(nullptr);
    if (chained) HIPCHK(c, timed_event_wait(c->wait_ms[3], f.uploaded));
    // -- independent of the previous frame ---------------------------------------------------------------------
    // Id-map path only (debug mode, POPPY_HIP_IDMAP, oversized tile lists).  The id map is not cleared between frames: every
    // frame writes its ids above a tag that grows from frame to frame, and its warp kernel reads everything else as "no
    // triangle" (kernels.h: launch_raster).  A memset is needed for a slot's first frame, when the tags run out (every 2047
    // frames), and around debug frames, which keep a plain map for poppy_hip_debug_fetch.
    if (!bin_warp) {
        if (c->debug || f.map_tag == 0 || f.map_tag >= kIdTagMax) {
            HIPCHK(c, hipMemsetAsync(f.triMap, 0, (size_t)W * H * 4, s));
            f.map_tag = 0;
        }
        if (!c->debug) ++f.map_tag;
    }
    const uint32_t id_base = (uint32_t)f.map_tag << kIdTagShift;
    if (all_marks) tm.mark("upload+clear");
    if (!bin_warp) launch_raster(d.tri, d.edges, d.work, pr.n_work, f.triMap, W, H, id_base, s);
    if (all_marks) tm.mark("raster");
    // -- chained mode: corrected1 is the previous frame (src/poppy.hpp:217) -------------------------------------
    if (c->cur1_ready && c->cur1_stream != s) HIPCHK(c, hipStreamWaitEvent(s, c->cur1_ready, 0));
    WarpExtras ex;
    ex.id_base = id_base;
    // lbmask (level 0 of pyrM) rides along with the warp only where the blend kernels cannot read it through m2
    ex.m2 = c->lazy_mask ? nullptr : c->m2; ex.mask = f.pyrM; ex.alpha = 1.0 - mask; ex.beta = -mask;
    ex.out_pitch = c->levels[0].pitch;
    if (c->timing == 2) {       // the dispatch's own begin / end timestamps: no marker packets in the stream
        // A stamped dispatch still costs the frame loop ~5 us (it completes through a signal the host can read: 2.6 % of a
        // chained 1080p frame when every launch is stamped), so one launch in kWarpStampStride carries the stamps; the
        // stride is coprime with the usual sequence lengths, so over a few sequences every frame position is sampled.
        static const int stride = getenv("POPPY_HIP_WARP_STAMP_STRIDE") ? std::max(1, atoi(getenv("POPPY_HIP_WARP_STAMP_STRIDE"))) : kWarpStampStride;
        const bool stamp = (c->warp_seq++ % (unsigned)stride) == 0;
        hipEvent_t t0 = stamp ? tm.take(nullptr) : nullptr, t1 = stamp ? tm.take("warp") : nullptr;
        launch_frame_warp(c, f, pr, d, ex, s, t0, t1);
    } else {
        if (!all_marks) tm.mark(nullptr);
        launch_frame_warp(c, f, pr, d, ex, s);
        tm.mark("warp");
    }
    if (bin_warp) {
        c->last_warp.rec = d.rec; c->last_warp.tile_data = f.tile_data; c->last_warp.tile_bytes = c->tile_bytes;
        c->last_warp.toff = d.toff; c->last_warp.tile_w = pr.tile_w; c->last_warp.c1 = c->cur1; c->last_warp.c2 = c->c2;
        c->last_warp.tr1 = f.tr1; c->last_warp.tr2 = f.tr2; c->last_warp.ex = ex; c->last_warp.valid = true;
    } else c->last_warp.valid = false;
    // The frame's completion event rides on its last dispatch when the kernels are launched one by one: an event record of
    // its own behind the last kernel leaves the stream idle for ~6 us before the next frame's first kernel.
    static const bool done_packet = getenv("POPPY_HIP_DONE_PACKET") != nullptr;
    const bool done_rides = !use_graph && !all_marks && !done_packet;
    // PAL8_SEQ: the frame's pass — behind the captured body on the same stream (the body stays BGR: the store address differs per frame), or as the body's last launch
    uint8_t* seq_dst = nullptr;
    if (seq_wanted(c) && !(seq_dst = seq_next_place(c))) return fail(c, POPPY_E_STATE, "more frames than the sequence was opened for");
    if (use_graph) { HIPCHK(c, hipGraphLaunch(f.body, s)); if (seq_dst) { int rc = seq_pass(c, slot_bgr(f, frame_wants_geom(c)), seq_dst, s, nullptr); if (rc) return rc; } }
    else { int rc = enqueue_body(c, f, s, all_marks ? &tm : nullptr, (float)(1.0 - amount), c->debug, done_rides ? f.done : nullptr, chained, seq_dst); if (rc) return rc; }
    HIPCHK(c, hipGetLastError());
    if (!done_rides) HIPCHK(c, hipEventRecord(f.done, s));
    c->last_slot = fi;
    if (chain) {                                   // src/poppy.hpp:217-218
        c->cur1 = f.out;
        c->cur1_ready = f.done;
        c->cur1_stream = s;
        c->pts1 = pr.morphed;
    }
    return POPPY_OK;
}

int submit_frame(poppy_hip_ctx* c, double mask, bool chain) {
    const int fi = pick_slot(c);
    c->next_slot = (fi + 1) % (int)c->slots.size();
    ++c->frame_seq;
    SlotPrep& pr = c->slot_preps[fi];
    if (!(pr.valid && pr.seq == c->frame_seq && pr.chained && chain)) {             // (not prepared ahead for THIS call: both halves now)
        drop_slot_preps(c);
        int rc = prepare_slot(c, c->plan, mask, chain, fi); if (rc) return rc;
    }
    return render_slot(c, fi, chain);
}

// Chained frames only: the first half of the NEXT frame, launched behind the frame just submitted.  `plan` is that frame's; its slot is the one submit_frame will pick.
int prepare_ahead(poppy_hip_ctx* c, const FramePlan& plan, double mask) {
    static const bool off = getenv("POPPY_HIP_NO_PREPARE_AHEAD") != nullptr;
    if (off || c->debug || c->timing != 0 || c->slots.size() < 3) return POPPY_OK;
    const int fi = pick_slot(c);
    const int rc = prepare_slot(c, plan, mask, true, fi);
    if (rc == POPPY_OK) c->slot_preps[fi].seq = c->frame_seq + 1;
    return rc;
}

// The frame body's last stage on a caller's float image (include/poppy_hip.h): the same launcher, threshold and bound as enqueue_body's call, the kernel named by
// `form`.  Buffers of the call's own: no pair needs to be resident and none is disturbed beyond the kept chain state.
int poppy_hip_unsharp_frame(poppy_hip_ctx* c, const float* src, int W, int H, int pitch, float amount, int form, int amount_on_device,
                            uint8_t* dst, float* dst_f32_or_null) {
    if (!c) return POPPY_E_ARG;
    if (!src || !dst || W <= 0 || H <= 0 || pitch < W || form < kUnsharpAuto || form > kUnsharpSeparable || (amount_on_device != 0 && amount_on_device != 1))
        return fail(c, POPPY_E_ARG, "bad unsharp_frame arguments");
    if (form == kUnsharpStream && !unsharp_stream_takes(W, H)) return fail(c, POPPY_E_UNSUPPORTED, "the streaming unsharp kernel takes frames from 64 x 16 pixels up");
    if (form == kUnsharpTile && (W < 2 || H < 2)) return fail(c, POPPY_E_UNSUPPORTED, "the tile unsharp kernel takes frames from 2 x 2 pixels up");
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    const size_t n_src = (size_t)pitch * H * 3, n_out = (size_t)W * H * 3;
    const bool separable = form == kUnsharpSeparable || W < 2 || H < 2;
    float *d_src = nullptr, *d_tmp = nullptr, *d_diff = nullptr, *d_outF = nullptr, *d_amount = nullptr;
    uint8_t* d_out = nullptr;
    hipError_t e = hipMalloc((void**)&d_src, n_src * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, n_out);
    if (e == hipSuccess && separable) e = hipMalloc((void**)&d_tmp, n_out * 4);
    if (e == hipSuccess && separable) e = hipMalloc((void**)&d_diff, n_out * 4);
    if (e == hipSuccess && dst_f32_or_null) e = hipMalloc((void**)&d_outF, n_out * 4);
    if (e == hipSuccess && amount_on_device) e = hipMalloc((void**)&d_amount, 4);
    // the source goes up with its pitch: the padding pixels are on the device, where a kernel that read them would show it
    if (e == hipSuccess) e = hipMemcpyAsync(d_src, src, n_src * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && d_amount) e = hipMemcpyAsync(d_amount, &amount, 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        // amount_on_device: as in a captured body, the argument is 0 and the value is the buffer's (the separable kernels take the argument: kernels.h)
        launch_unsharp(d_src, d_tmp, d_diff, d_out, d_outF, W, H, d_amount && !separable ? 0.f : amount, d_amount, (float)0.3, c->stream, nullptr, pitch, form);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(dst, d_out, n_out, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && d_outF) e = hipMemcpyAsync(dst_f32_or_null, d_outF, n_out * 4, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);      // also on failure: `amount` and the host images are read until the copies have run
    if (e == hipSuccess) e = es;
    void* bufs[] = {d_src, d_out, d_tmp, d_diff, d_outF, d_amount};
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (e != hipSuccess) { c->err = std::string("unsharp_frame: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}
