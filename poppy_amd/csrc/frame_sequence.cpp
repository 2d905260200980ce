// frame_sequence.cpp — the multi-frame driver (frame_sequence.h): the plans of a sequence on the context's planner team, one frame and a sequence of frames on the
// resident pair, and the download pump that hands the frames of a sequence to its writer.  What a frame launches is frame_render.cpp's.
#include "context.h"
#include <chrono>

std::atomic<int> g_live_contexts{0};

// what every frame of the resident pair needs: the pair, and point pairs to plan a mesh from
static int frames_ready(poppy_hip_ctx* c) {
    if (!c->pair_ready) return fail(c, POPPY_E_STATE, "no pair loaded");
    if (c->pts1.empty()) return fail(c, POPPY_E_NOMATCH, "no point pairs (use poppy_hip_dissolve)");
    return POPPY_OK;
}

// one frame on the resident pair; result in frame[slot]
int render_frame(poppy_hip_ctx* c, double shape, double mask, bool chain) {
    int rc = frames_ready(c); if (rc) return rc;
    rc = plan_frame(c->W, c->H, c->pts1, c->pts2, shape, c->plan);
    if (rc) return fail(c, POPPY_E_RANGE, "point outside the image rectangle (Subdiv2D::insert would throw)");
    if (warp_bin_geometry(c->W, c->H)) { const int tw = warp_bin_tile_width(c->W, c->H); build_tile_bins(c->plan, c->W, c->H, tw, 1024 / tw, c->bins_cap); }
    return submit_frame(c, mask, chain);
}

// Multi-frame calls plan on a small pool of host threads: only the POINT chain is sequential in chained mode
// (src/poppy.hpp:178-179,218: srcPoints1 <- morphedPoints), and that is a few hundred multiply-adds per frame; the
// triangulation and matrix work of the frames is independent once each frame's input points are known.
constexpr int kPlanThrew = -1000;          // rcs[] marker: the planner of that frame threw

static bool same_points(const std::vector<P2f>& a, const std::vector<P2f>& b) {           // bit for bit
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(P2f)) == 0);
}
bool end_seq_plans(poppy_hip_ctx* c) {
    if (!c->seq_plans) return true;
    c->seq_plans->next.store(c->seq_plans->n);                     // the planners stop at their next frame
    const bool ok = c->planners.wait();
    c->seq_plans.reset();
    return ok;
}
static SeqPlans* start_seq_plans(poppy_hip_ctx* c, const double* shape, int n, bool chain) {
    const int W = c->W, H = c->H;
    SeqPlans* sp = new SeqPlans(n);
    c->seq_plans.reset(sp);                                       // (the previous ones have been ended: end_seq_plans)
    sp->W = W; sp->H = H; sp->chain = chain; sp->shape.assign(shape, shape + n); sp->pts1_at_start = c->pts1; sp->pts2 = c->pts2;
    std::vector<std::vector<P2f>>& src1 = sp->src1;
    src1[0] = c->pts1;
    if (chain)
        for (int j = 0; j + 1 < n; ++j) {                            // morph_points + clip_points of frame j
            const float s = (float)shape[j];
            std::vector<P2f> a = src1[j], b = c->pts2;
            clip_points_ref(a, W, H); clip_points_ref(b, W, H);
            std::vector<P2f>& m = src1[j + 1];
            m.resize(a.size());
            for (size_t i = 0; i < a.size(); ++i) {
                m[i].x = (float)((1.0 - s) * a[i].x + s * b[i].x);
                m[i].y = (float)((1.0 - s) * a[i].y + s * b[i].y);
            }
            clip_points_ref(m, W, H);
        }
    // planner threads of this call: at most 16, and the contexts alive in this process share the host's threads between them (a pool of 3 contexts
    // x 8 devices would otherwise park ~400 planner threads; the planners of one context keep up with its GPU from ~4 threads: 0.3 ms per plan)
    const int alive = std::max(1, g_live_contexts.load());
    const int share = std::max(4, ((int)std::thread::hardware_concurrency() - 1) / alive);
    const int nthreads = std::max(1, std::min({n, 16, share, (int)std::thread::hardware_concurrency() - 1}));
    const int bin_tw = warp_bin_geometry(W, H) ? warp_bin_tile_width(W, H) : 0;
    const size_t bins_cap = c->bins_cap;
    auto worker = [sp, W, H, bin_tw, bins_cap, chain]() {
        for (;;) {
            const int j = sp->next.fetch_add(1);
            if (j >= sp->n) return;
            // a planner that throws (std::bad_alloc is the case that can happen) must still publish its frame: the calling thread spins on ready[j]
            try {
                sp->rcs[j] = plan_frame(W, H, chain ? sp->src1[j] : sp->src1[0], sp->pts2, sp->shape[j], sp->plans[j]);
                if (!sp->rcs[j] && bin_tw) build_tile_bins(sp->plans[j], W, H, bin_tw, 1024 / bin_tw, bins_cap);
            } catch (...) { sp->rcs[j] = kPlanThrew; }
            sp->ready[j].store(1, std::memory_order_release);
        }
    };
    c->planners.run(nthreads, worker);                            // persistent threads (worker.h): parked between calls
    return sp;
}
void start_default_seq_plans(poppy_hip_ctx* c) {
    static const bool off = getenv("POPPY_HIP_NO_PLAN_AHEAD") != nullptr;
    if (SeqPlans* old = c->seq_plans.get()) {
        // The previous pair's plans were never taken: this caller loads pairs without rendering the default sequence in between (a set-up timing loop, a caller
        // of single frames).  Planning ahead for it only burns host threads beside its next set-up (0.3 ms per set-up in such a loop), and waiting for planners in
        // mid-frame cost another 0.2 ms: they are told to stop and left to finish, and no plans are started for a pair until a multi-frame call has been seen again.
        c->plan_ahead_credit = false;
        old->abandoned = true;
        old->next.store(old->n);
        if (!c->planners.idle()) return;
    }
    (void)end_seq_plans(c);
    if (!c->plan_ahead_credit) return;
    const int N = c->cfg.number_of_frames;
    if (off || N < 2 || c->pts1.empty() || c->debug) return;
    std::vector<double> ratio(N);
    for (int j = 0; j < N; ++j) ratio[j] = poppy_frame_ratio(j, N, -1.0);
    start_seq_plans(c, ratio.data(), N, true);
}

using clk = std::chrono::steady_clock;
static double lap(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

// Frame hand-off.  The download of a frame runs on its own stream into a ring of R pinned buffers while the GPU renders the
// frames behind it, and the writer gets frames in order, R - 1 downloads behind.  A copy whose start depends on an event of
// ANOTHER stream is launched by the runtime's asynchronous-event thread when that event fires; with two contexts rendering and
// downloading at once those launches crawled (22 GB/s together against 52 GB/s for copies without a dependency:
// tools/experiments/d2h_raw.py, overlap_probe.py).  So the host waits for frame j-1 itself — frame j is already queued, the GPU
// never idles for it — and then issues a copy that depends on nothing.  (POPPY_HIP_DL_DEVWAIT=1: the dependent form.)  The copy is
// the runtime's: a kernel of ours storing the frame into the mapped ring costs the frame kernels beside it far more (3.7k frames/s
// against 5.8k, whatever its geometry: shader stores over PCIe hold up the other kernels' stores, profiles/r02_notes.md section 7).
//
// Round 6: a frame copy goes to the stream of its pinned ring buffer, which carries nothing else, and NO event is recorded behind it — whoever needs the copy
// finished synchronises that stream.  An event record behind a copy is a marker packet that waits, in one of the process's four hardware queues, for the copy's
// signal, and every kernel of every stream mapped to that queue waits with it for the length of a frame copy (~120 us): a pool of six with the writer 6.2 -> 6.6-6.9k
// frames/s (7.4-7.6k on the runtime bundled with torch), one context 5.2 -> 5.4k, the 480-frame phase-mode job 6.0-6.2 -> 7.2-7.5k (profiles/r06_dl_streams.txt).
// POPPY_HIP_DL_EVENTS=1: one download stream + an event per copy, as until round 5.
struct FramePump {
    poppy_hip_ctx* c;
    poppy_write_cb write; void* user;
    int fmt;                               // the writer's format: the frame body converts the frame into the slot's buffer of that format (enqueue_body)
    WriterGeom geom;                       // the writer's geometry: what it is told, and what sizes row and frame_bytes
    size_t row, frame_bytes;               // (GIF: a coded frame goes to the writer with stride 0; frame_bytes is its capacity, which sizes the pinned ring — a frame's copy moves its own length)
    bool dev_wait, dl_streams;
    WriterRing ring;                       // (frames 0 .. ring.issued - 1: their downloads are queued)
    std::vector<int> slot_of;              // the slot frame k was rendered into
    double ms_done = 0, ms_deliver = 0;    // the calling thread's waits for frames to finish and for downloads (POPPY_SEQ_TIMING)
    int rc = POPPY_OK;

    bool issue_download(int k) {
        FrameSlot& f = c->slots[slot_of[k]];
        const int r = k % ring.R;
        const auto t0 = clk::now();
        // (GIF: the host waits in every form: k_gif_pack has stored the frame's length into the slot's pinned word by then, and the copy moves that many bytes)
        hipError_t e = dev_wait && !format_traits(fmt)->coded() ? hipStreamWaitEvent(c->dl_stream, f.done, 0) : hipEventSynchronize(f.done);
        ms_done += lap(t0);
        size_t copy_bytes = frame_bytes;
        if (e == hipSuccess && !slot_frame_length(f, fmt, frame_bytes, &copy_bytes)) { c->err = "the coded frame's length is outside its bounds"; rc = POPPY_E_DEVICE; return false; }
        if (dl_streams) {
            hipStream_t ds = nullptr;
            if (e == hipSuccess) e = ring.stream(c, k, &ds);
            if (e == hipSuccess) e = hipMemcpyAsync(ring.buffer(k), slot_frame(f, fmt, geom), copy_bytes, hipMemcpyDeviceToHost, ds);
            f.dl_pending = true; f.dl_ring_idx = r;
            if (e != hipSuccess) { c->err = std::string("frame download: ") + hipGetErrorString(e); rc = POPPY_E_DEVICE; return false; }
            return true;
        }
        f.dl_ring_idx = -1;
#ifdef POPPY_EXPERIMENTS
        static const bool skip_copy = getenv("POPPY_DL_SKIP_COPY") != nullptr;      // timing experiment: every wait and event of the writer path, no bytes moved (wrong frames)
        if (!skip_copy)
#endif
        if (e == hipSuccess) e = hipMemcpyAsync(ring.buffer(k), slot_frame(f, fmt, geom), copy_bytes, hipMemcpyDeviceToHost, c->dl_stream);
        if (e == hipSuccess) e = hipEventRecord(c->dl_done[r], c->dl_stream);
        if (e == hipSuccess) e = hipEventRecord(f.downloaded, c->dl_stream);          // the slot's own: ring events are re-recorded every R frames
        f.dl_pending = true;
        if (e != hipSuccess) { c->err = std::string("frame download: ") + hipGetErrorString(e); rc = POPPY_E_DEVICE; return false; }
        return true;
    }
    void deliver() {
        const auto t0 = clk::now();
        uint8_t* frame = nullptr;
        if (ring.deliver_next(c, !dl_streams, &frame) != hipSuccess) { c->err = "frame download failed"; rc = POPPY_E_DEVICE; return; }
        ms_deliver += lap(t0);
        write(user, frame, geom.w, geom.h, row);
    }
    // the downloads of the frames before `upto` are queued, each behind the delivery that frees its ring buffer
    void pump(int upto) {
        while (ring.issued < upto && rc == POPPY_OK) {
            while (ring.issued - ring.written >= ring.R && rc == POPPY_OK) deliver();
            if (rc == POPPY_OK && issue_download(ring.issued)) ++ring.issued;
        }
    }
    // The slot frame j renders into may still hold a frame whose download has not been issued (few slots, or every frame
    // landing in the one slot that does not hold corrected1): that copy goes out first; submit_frame then waits for it.
    void free_slot_for(int j) {
        int ps = c->next_slot;
        if (c->slots[ps].out == c->cur1) ps = (ps + 1) % (int)c->slots.size();
        int last_user = -1;
        for (int k = ring.issued; k < j; ++k) if (slot_of[k] == ps) last_user = k;
        pump(last_user + 1);
    }
    void drain(int n) {                    // the last frame(s), then the ring
        pump(n);
        while (ring.written < n && rc == POPPY_OK) deliver();
    }
};

static int render_sequence_frames(poppy_hip_ctx* c, const double* shape, const double* mask, int n, bool chain, poppy_write_cb write, void* user) {
    const int W = c->W, H = c->H;
    const bool seq = writer_wants_sequence(c, write != nullptr);
    if (n >= 2) c->plan_ahead_credit = true;                       // a caller of sequences: the next pair loader plans ahead again (start_default_seq_plans)
    // the plans a pair loader started for exactly these frames on exactly these points, or new ones
    SeqPlans* sp = c->seq_plans.get();
    if (!(sp && !sp->abandoned && sp->n == n && sp->chain == chain && sp->W == W && sp->H == H && same_points(sp->pts1_at_start, c->pts1) && same_points(sp->pts2, c->pts2) &&
          std::equal(shape, shape + n, sp->shape.begin()))) {
        (void)end_seq_plans(c);
        sp = start_seq_plans(c, shape, n, chain);
    }
    static const bool dev_wait = getenv("POPPY_HIP_DL_DEVWAIT") != nullptr;
    static const bool dl_streams = getenv("POPPY_HIP_DL_EVENTS") == nullptr && !dev_wait;
    const int fmt = writer_format(c, write != nullptr);
    const WriterGeom geom = writer_geom(c, write != nullptr);
    for (const FrameSlot& f : c->slots)
        if (!slot_format_ready(c, f, fmt, geom)) return fail(c, POPPY_E_STATE, "the frame format's buffers are not allocated for this pair");
    FramePump dlp{c, write, user, fmt, geom, writer_stride(fmt, geom.w), poppy_frame_bytes(fmt, geom.w, geom.h), dev_wait, dl_streams};
    dlp.slot_of.assign(n, -1);
    const bool dl = write && !seq;                                // frames are downloaded and handed over as they finish
    int rc = POPPY_OK;
    if (dl) rc = dlp.ring.open(c, dlp.frame_bytes, true);
    c->writer_attached = write != nullptr;                        // (phase-mode frames pick their streams by it: choose_frame_stream)
    static const bool seq_times = getenv("POPPY_SEQ_TIMING") != nullptr;      // where the calling thread's time goes, on stderr
    double ms_plan = 0, ms_submit = 0;
    const auto t_seq = clk::now();
    const double w0[4] = {c->wait_ms[0], c->wait_ms[1], c->wait_ms[2], c->wait_ms[3]};
    const int pal8_lag = format_traits(fmt)->slot_raster() == kRasterPal8 ? std::max(0, (int)c->slots.size() - 2) : 0;
    // plan, free the slot, submit, prepare ahead, pump
    for (int j = 0; j < n && rc == POPPY_OK; ++j) {
        const auto t_plan = clk::now();
        while (!sp->ready[j].load(std::memory_order_acquire)) std::this_thread::yield();
        ms_plan += lap(t_plan);
        if (sp->rcs[j] == kPlanThrew) { rc = fail(c, POPPY_E_DEVICE, "frame planner failed (out of memory?)"); break; }
        if (sp->rcs[j]) { rc = fail(c, POPPY_E_RANGE, "point outside the image rectangle (Subdiv2D::insert would throw)"); break; }
        c->plan = std::move(sp->plans[j]);
        if (chain) c->pts1 = sp->src1[j];
        if (dl) { dlp.free_slot_for(j); if ((rc = dlp.rc) != POPPY_OK) break; }
        const auto t_sub = clk::now();
        rc = submit_frame(c, mask[j], chain);
        // chained frames: the NEXT frame's plan goes up and is expanded now, behind this frame's launches (the wait for it at the head of the next
        // submit_frame then finds it done); only when its plan is ready — the planners are normally far ahead
        if (rc == POPPY_OK && chain && j + 1 < n && sp->ready[j + 1].load(std::memory_order_acquire) && sp->rcs[j + 1] == 0) rc = prepare_ahead(c, sp->plans[j + 1], mask[j + 1]);
        ms_submit += lap(t_sub);
        if (rc != POPPY_OK) break;
        dlp.slot_of[j] = c->last_slot;
        // frames whose download can be issued now.  A PAL8 frame is complete one palette build (several frame times) behind its BGR: waiting for frame
        // j - 1 here would hold back frame j + 1 for that long, so under PAL8 the downloads trail as far as the slots allow (free_slot_for sends
        // what a slot's reuse forces out) and the conversions of that many frames run beside each other.
        if (dl) { dlp.pump((dev_wait ? j + 1 : j) - pal8_lag); rc = dlp.rc; }
    }
    if (dl && rc == POPPY_OK) { dlp.drain(n); rc = dlp.rc; }
    c->writer_attached = false;
    drop_slot_preps(c);                    // (a frame prepared ahead and never rendered — an error exit — must not meet a later call)
    // on an error the planners stop at their next frame
    if (!end_seq_plans(c) && rc == POPPY_OK) rc = fail(c, POPPY_E_DEVICE, ("frame planner thread: " + c->planners.error()).c_str());
    if (seq_times)
        fprintf(stderr, "sequence of %d frames: %.2f ms; waiting for plans %.2f, submit_frame %.2f (of which waiting for: the slot's download %.2f, its pinned plan %.2f, "
                "its last frame %.2f, upload + expansion %.2f), waiting for frames to finish %.2f, waiting for downloads %.2f ms\n",
                n, lap(t_seq), ms_plan, ms_submit, c->wait_ms[0] - w0[0], c->wait_ms[1] - w0[1], c->wait_ms[2] - w0[2], c->wait_ms[3] - w0[3], dlp.ms_done, dlp.ms_deliver);
    return rc;
}

// PAL8_SEQ: the frames go through the pass into the sequence store and to the writer when all are there — of this call's own sequence, or of the one its caller
// opened and ends (in_open_seq: poppy_hip_render_phases).  Opened first: its limits refuse before anything is rendered.  Every way out of the frames' loop
// comes back here, so a sequence this call opened is finished or aborted, never left open.
int render_sequence(poppy_hip_ctx* c, const double* shape, const double* mask, int n, bool chain, poppy_write_cb write, void* user, bool in_open_seq) {
    if (int rc = frames_ready(c)) return rc;
    if (n <= 0) return POPPY_OK;
    const bool own_seq = writer_wants_sequence(c, write != nullptr) && !in_open_seq;
    if (own_seq) { int rc = seq_begin(c, n); if (rc) return rc; }
    int rc = render_sequence_frames(c, shape, mask, n, chain, write, user);
    c->writer_attached = false;
    if (own_seq) { if (rc == POPPY_OK) rc = seq_finish(c, write, user); else seq_abort_keep_error(c); }
    return rc;
}

// a writer that only counts the frames it is handed (user: a long long, or null)
extern "C" void poppy_count_frames_cb(void* user, const uint8_t*, int, int, size_t) { if (user) ++*(long long*)user; }

