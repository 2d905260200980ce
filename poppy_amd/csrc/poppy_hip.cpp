// poppy_hip.cpp — context life cycle, HBM layout, the pair loaders and the C entry points of include/poppy_hip.h.  The per-frame path is frame_render.cpp,
// the multi-frame driver frame_sequence.cpp.
//
// Host C++ (as the reference's own morph driver is, src/poppy.hpp:46-248) calling the hand-written
// gfx950 kernels of kernels_*.hip.  Per pair everything stays resident in HBM; per frame the host only
// plans the mesh (frame_plan.cpp, ~1k triangles) and uploads ~100 KB through a pinned ring.
//
// HBM layout for a W x H pair (P = W*H):
//   c1, c2            u8x3   3P each     sources (c1 is replaced by the previous frame in chained mode)
//   m2                f32    4P          1 - gray(gabor2), loop invariant (algo.cpp:250-252)
// and per frame SLOT (POPPY_HIP_SLOTS of them, 4 unless it says otherwise; chained frames all run on the context's stream with their plan upload and
// raster expansion on the copy stream, independent — phase-mode — frames each on their slot's stream, several in flight at once: prepare_slot):
//   triMap            i32    4P          triangle id per pixel
//   tr1, tr2          u8x3   3P each     warped sources (never widened to float in memory)
//   pyrL, pyrR        f32x3  ~4P each    Gaussian levels 1..levels of the warped sources
//   pyrM              f32    ~5.3P       mask levels 0..levels
//   pyrB              f32x3  ~16P        blended levels; level 0 is lapBlend
//   out               u8x3   3P          the frame (chained mode feeds it to the next slot as c1)
// No CPU fallback exists in this library: every entry point either runs the kernels or fails.
#include "context.h"

static std::string g_create_error;

// Streams and hardware queues.  The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless the variable
// says otherwise); streams that share a queue run in order, and queues are handed out — and spread over the command processor's
// pipes — in the order the streams are created.  Which queue the frame-download stream gets decides what the writer hand-off costs:
// created lazily as a context's fifth stream it got, with 5 or more queues allowed, a queue of its own that delayed EVERY dispatch of
// the rendering stream by ~40 us while a copy was pending (chained 1080p loop with writer: 3.9k frames/s against 5.9k; kernels of 8 us
// show up as 45 us in the trace), and with fewer than 4 it shared the rendering stream's queue (4.7k).  So a context creates its three
// hot streams first and in this order — rendering, plan upload, frame download — and the library leaves the queue count alone:
// 5.7-6.0k frames/s with 4, 5, 8 or 16 queues, with the image's runtime (downloads on the SDMA engines) and with the one bundled in
// the torch wheel (blit kernels).  Measurements: profiles/r02_notes.md section 7, tools/experiments/hwq_matrix.sh, hwq_sweep.sh, hwq_sweep4.sh, writer_gap.py.


extern "C" {

void poppy_settings_default(poppy_settings* s) {
    s->number_of_frames = 60; s->match_tolerance = 1.0; s->max_keypoints = 300; s->pyramid_levels = 64; s->enable_radial_mask = 0; s->enable_auto_align = 0;
}
const char* poppy_hip_create_error(void) { return g_create_error.c_str(); }
const char* poppy_hip_last_error(const poppy_hip_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

poppy_hip_ctx* poppy_hip_create(int device, const poppy_settings* settings) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { g_create_error = "no HIP device (libpoppy_hip has no CPU fallback)"; return nullptr; }
    if (device < 0 || device >= n) { g_create_error = "device index out of range"; return nullptr; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { g_create_error = "hipGetDeviceProperties failed"; return nullptr; }
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        g_create_error = std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only";
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return nullptr; }
    poppy_hip_ctx* c = new poppy_hip_ctx();
    c->device = device;
    c->max_grid_y = prop.maxGridSize[1];
    if (settings) c->cfg = *settings; else poppy_settings_default(&c->cfg);
    c->foreground.radial_mask_on = c->foreground_b.radial_mask_on = c->cfg.enable_radial_mask != 0;      // src/extractor.cpp:178-197
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { g_create_error = "hipStreamCreate failed"; delete c; return nullptr; }
    if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) { g_create_error = "hipStreamCreate failed"; delete c; return nullptr; }
    if (hipStreamCreateWithFlags(&c->dl_stream, hipStreamNonBlocking) != hipSuccess) { g_create_error = "hipStreamCreate failed"; delete c; return nullptr; }
    for (hipEvent_t& e : c->dl_done)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { g_create_error = "hipEventCreate failed"; delete c; return nullptr; }
    (void)hipEventCreateWithFlags(&c->inputs_ready, hipEventDisableTiming);
    int k = 4;                                             // frames in flight
    if (const char* e = getenv("POPPY_HIP_SLOTS")) k = atoi(e);
    c->slots.resize(std::max(2, std::min(k, 8)));
    c->slot_preps.resize(c->slots.size());
    for (FrameSlot& f : c->slots) {
        // (hipEventDisableSystemFence on `done` was measured: +0.6-1 % frames/s; not used, because frame downloads to the
        // host are ordered by this event)
        if (hipEventCreateWithFlags(&f.downloaded, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&f.uploaded, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&f.done, hipEventDisableTiming) != hipSuccess) {
            g_create_error = "hipStreamCreate failed"; delete c; return nullptr;
        }
    }
    g_live_contexts.fetch_add(1);
    return c;
}

static void free_pair(poppy_hip_ctx* c) {
    c->last_warp.valid = false;                     // its pointers go with the pair's buffers
    void* bufs[] = {c->arena, c->c2_raw, c->gabor2, c->d_levels};
    for (void* b : bufs) if (b) (void)hipFree(b);
    c->arena = nullptr; c->arena_bytes = 0;
    c->c1 = c->c2 = c->c2_raw = nullptr; c->gabor2 = c->m2 = nullptr; c->d_levels = nullptr;
    for (FrameSlot& f : c->slots) {
        void* fb[] = {f.tr1, f.tr2, f.out, f.pyrL, f.pyrR, f.pyrM, f.pyrB, f.tmp, f.diff, f.unsharpF, f.triMap};
        for (void* b : fb) if (b) (void)hipFree(b);
        f.tr1 = f.tr2 = f.out = nullptr; f.pyrL = f.pyrR = f.pyrM = f.pyrB = f.tmp = f.diff = f.unsharpF = nullptr; f.triMap = nullptr;
        free_slot_format_pair(f.fmt);
    }
    for (FrameSlot& f : c->slots) {
        if (f.body) { (void)hipGraphExecDestroy(f.body); f.body = nullptr; }
        if (f.h_blob) (void)hipHostFree(f.h_blob);
        if (f.d_blob) (void)hipFree(f.d_blob);
        if (f.tile_data) (void)hipFree(f.tile_data);
        f.h_blob = nullptr; f.d_blob = nullptr; f.tile_data = nullptr;
    }
    c->max_tris = 0; c->W = c->H = 0; c->pair_ready = false;
}

void poppy_hip_destroy(poppy_hip_ctx* c) {
    if (!c) return;
    g_live_contexts.fetch_sub(1);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)poppy_hip_comm_free(c);
    for (FrameSlot& f : c->slots)
        for (hipStream_t st : {f.stream, f.own_stream, f.fmt.fmt_stream}) if (st) (void)hipStreamSynchronize(st);
    free_pair(c);
    for (FrameSlot& f : c->slots) {
        if (f.done) (void)hipEventDestroy(f.done);
        if (f.downloaded) (void)hipEventDestroy(f.downloaded);
        if (f.uploaded) (void)hipEventDestroy(f.uploaded);
        if (f.own_stream) (void)hipStreamDestroy(f.own_stream);
        free_slot_format_ctx(f.fmt);
    }
    if (c->inputs_ready) (void)hipEventDestroy(c->inputs_ready);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->dl_stream) { (void)hipStreamSynchronize(c->dl_stream); (void)hipStreamDestroy(c->dl_stream); c->dl_stream = nullptr; }
    for (hipStream_t& st : c->dl_ring) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); st = nullptr; }
    if (c->aux_stream) { (void)hipStreamSynchronize(c->aux_stream); (void)hipStreamDestroy(c->aux_stream); }
    (void)end_seq_plans(c);
    if (c->setup_ev) (void)hipEventDestroy(c->setup_ev);
    if (c->c2_up_ev) (void)hipEventDestroy(c->c2_up_ev);
    for (hipEvent_t e : c->dl_done) if (e) (void)hipEventDestroy(e);
    for (auto& m : c->marks) (void)hipEventDestroy(m.ev);
    (void)hipStreamSynchronize(c->copy_stream);
    if (c->d_align) (void)hipFree(c->d_align);
    for (void* p : {(void*)c->bm_canvas, (void*)c->bm_tmp, (void*)c->bm_taps, (void*)c->list_img[0], (void*)c->list_img[1]}) if (p) (void)hipFree(p);
    if (c->d_comm_scratch) (void)hipFree(c->d_comm_scratch);
    free_context_format(c);
    c->aligner.release();
    c->ransac_scratch.release();
    for (DeviceBuffer* b : {&c->denoise.table, &c->denoise.stage, &c->denoise.list_img[0], &c->denoise.list_img[1]}) b->release();
    (void)hipStreamDestroy(c->copy_stream);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

int poppy_warp_records(const float* inv1, const float* inv2, int n_tris, int width, int height, float* records) {
    if (n_tris < 0 || width < 1 || height < 1 || !records || (n_tris > 0 && (!inv1 || !inv2))) return POPPY_E_ARG;
    return pack_warp_records(inv1, inv2, n_tris, width, height, records) ? 1 : 0;
}
int poppy_hip_last_warp_kind(poppy_hip_ctx* c) { return c ? (c->last_warp_bin ? 2 : c->last_warp_fast ? 1 : 0) : POPPY_E_ARG; }
int poppy_hip_last_pyramid_forms(poppy_hip_ctx* c, int* out, int cap) {
    if (!c || cap < 0 || (cap > 0 && !out)) return POPPY_E_ARG;
    if (c->pyr_forms.empty()) return POPPY_E_STATE;
    const int n = (int)c->pyr_forms.size() / 3;
    if (cap > 0) memcpy(out, c->pyr_forms.data(), (size_t)std::min(n, cap) * 3 * sizeof(int));
    return n;
}
int poppy_hip_warp_counts(poppy_hip_ctx* c, unsigned long long* fused, unsigned long long* tiled, unsigned long long* general) {
    if (!c) return POPPY_E_ARG;
    if (fused) *fused = c->n_warp_bin;
    if (tiled) *tiled = c->n_warp_fast;
    if (general) *general = c->n_warp_general;
    return POPPY_OK;
}
// Relaunches the last frame's fused raster + warp kernel `reps` times back to back on the context's stream, nothing else running, and
// returns the average time per launch between two events around the batch (milliseconds) — the kernel's duration as the kernel traces
// show it, without the per-dispatch stamps' overhead.  The relaunches write the same warped images again.
int poppy_hip_time_last_warp(poppy_hip_ctx* c, int reps, float* ms_per_launch) {
    if (!c || reps < 1 || !ms_per_launch) return POPPY_E_ARG;
    if (!c->last_warp.valid) return fail(c, POPPY_E_STATE, "no fused raster + warp launch to repeat");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = drain_frames(c); if (rc) return rc; }
    const auto& w = c->last_warp;
    hipEvent_t e0, e1;
    HIPCHK(c, hipEventCreate(&e0)); HIPCHK(c, hipEventCreate(&e1));
    launch_warp_bin(w.rec, w.tile_data, w.tile_bytes, w.toff, w.tile_w, w.c1, w.c2, w.tr1, w.tr2, c->W, c->H, w.ex, c->stream);      // warm
    HIPCHK(c, hipEventRecord(e0, c->stream));
    for (int i = 0; i < reps; ++i) launch_warp_bin(w.rec, w.tile_data, w.tile_bytes, w.toff, w.tile_w, w.c1, w.c2, w.tr1, w.tr2, c->W, c->H, w.ex, c->stream);
    HIPCHK(c, hipEventRecord(e1, c->stream));
    HIPCHK(c, hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms_per_launch = ms / (float)reps;
    return POPPY_OK;
}

int poppy_hip_mask_rider(poppy_hip_ctx* c) { return c ? (c->lazy_mask ? 0 : 1) : POPPY_E_ARG; }
int poppy_hip_set_debug(poppy_hip_ctx* c, int on) { if (!c) return POPPY_E_ARG; c->debug = on != 0; return POPPY_OK; }
int poppy_hip_set_timing(poppy_hip_ctx* c, int on) { if (!c) return POPPY_E_ARG; c->timing = on < 0 ? 0 : on; c->marks_used = 0; return POPPY_OK; }
void* poppy_hip_stream(poppy_hip_ctx* c) { return c ? (void*)c->stream : nullptr; }
int poppy_hip_sync(poppy_hip_ctx* c) { if (!c) return POPPY_E_ARG; HIPCHK(c, hipSetDevice(c->device)); return drain_frames(c); }

}  // extern "C"

// ---------------------------------------------------------------------------------------------
static int ensure_ring(poppy_hip_ctx* c, int n_points) {
    int need = plan_triangle_budget(n_points);
    if (need <= c->max_tris) return POPPY_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    c->last_warp.valid = false;                     // the plan blobs and tile entries it points into are reallocated below
    const int tw = warp_bin_tile_width(c->W, c->H);
    const size_t ntiles = tile_count(c->W, c->H, tw);
    c->bins_cap = tile_bins_capacity(n_points, c->W, c->H, tw);
    c->tile_bytes = warp_bin_data_bytes(ntiles, c->bins_cap);
    // (poppy_plan_blob_layout computes the same for the CPU test suite)
    const size_t bytes = plan_blob_capacity(need, c->H, ntiles, c->bins_cap);
    for (FrameSlot& f : c->slots) {
        if (f.body) { (void)hipGraphExecDestroy(f.body); f.body = nullptr; }      // it holds a pointer into the blob
        if (f.h_blob) (void)hipHostFree(f.h_blob);
        if (f.d_blob) (void)hipFree(f.d_blob);
        if (f.tile_data) (void)hipFree(f.tile_data);
        f.h_blob = f.d_blob = f.tile_data = nullptr;
        HIPCHK(c, hipMalloc((void**)&f.tile_data, c->tile_bytes));
        HIPCHK(c, hipHostMalloc((void**)&f.h_blob, bytes, hipHostMallocMapped));
        HIPCHK(c, hipHostGetDevicePointer(&f.h_blob_dev, f.h_blob, 0));
        HIPCHK(c, hipMalloc((void**)&f.d_blob, bytes));
    }
    c->blob_bytes = bytes;
    c->max_tris = need;
    return POPPY_OK;
}

int alloc_pair(poppy_hip_ctx* c, int W, int H) {
    { int rc = drain_frames(c); if (rc) return rc; }              // every pair loader comes through here: no frame still reads the old pair
    // PAL8 takes frames of at most 2^24 pixels (in the writer's geometry): refused before anything is allocated or any state changes, so the context keeps the pair it had
    // ... and a pair whose geometry does not admit the size set with poppy_hip_set_frame_size likewise
    if (const char* why = writer_refuses(c, c->frame_format, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    if (c->W == W && c->H == H && c->c1) return alloc_slot_format(c);      // (allocates only what is missing: nothing, unless an earlier attempt failed half-way)
    free_pair(c);
    c->pyr_forms.clear();
    if (c->cfg.pyramid_levels < 1 || c->cfg.pyramid_levels > 256) return fail(c, POPPY_E_UNSUPPORTED, "pyramid_levels must be in [1,256]");
    const size_t P = (size_t)W * H;
    const int L = c->cfg.pyramid_levels;
    c->levels.resize(L + 1);
    size_t off3 = 0, off1 = 0;
    int w = W, h = H;
    for (int i = 0; i <= L; ++i) {
        const int pitch = i == 1 ? level1_pitch(w, h, c->levels[0].pitch, W) : level_pitch(w, h);      // rows of the large levels begin on 16-byte boundaries (kernels.h)
        c->levels[i] = PyrLevel{w, h, off3, off1, pitch};
        off3 += (size_t)pitch * h * 3; off1 += (size_t)pitch * h;
        w = (w + 1) / 2; h = (h + 1) / 2;
    }
    const size_t P0 = (size_t)c->levels[0].pitch * H;             // pixels of a padded level-0 image (= P for widths that are multiples of 4)
    c->first_tail = L;
    static const size_t tail_px = getenv("POPPY_TAIL_PX") ? (size_t)atoi(getenv("POPPY_TAIL_PX")) : 600;
    for (int i = 1; i <= L; ++i)
        if ((size_t)c->levels[i].w * c->levels[i].h <= tail_px) { c->first_tail = i; break; }   // everything below runs in ONE workgroup: keep it small
    c->tail = build_pyr_tail_plan(c->levels.data(), std::min(c->first_tail, L), L);
    c->use_tail = c->tail.ok;
    static const bool rider = getenv("POPPY_HIP_LBMASK_RIDER") != nullptr;
    c->lazy_mask = !rider && c->cfg.pyramid_levels >= 1 && c->first_tail >= 1 && pyr_level0_vec_ok(W, H);
    if (c->use_tail) {
        if (!prepare_pyr_tail(c->tail.lds_bytes)) return fail(c, POPPY_E_DEVICE, "could not raise the tail kernel's LDS limit");
    } else {
        // A shallow pyramid (--pyramid 4 at 1080p ends at 120 x 68): every level goes through the per-level kernels and the
        // coarsest-level mix runs from global memory (blend.hpp simply loops `levels` times, any depth is legal).
        c->first_tail = L;
    }
    // +16: k_warp4 fetches footprints with 8-byte loads (6 bytes used), the last one may run 2 bytes past the image
    c->arena_bytes = pair_state_bytes(W, H);
    HIPCHK(c, hipMalloc((void**)&c->arena, c->arena_bytes));
    c->c1 = c->arena + kPairHeadBytes + 2 * (size_t)kPairMaxPoints * 8;
    c->c2 = c->c1 + pair_align(P * 3 + 16);
    c->m2 = (float*)(c->c2 + pair_align(P * 3 + 16));
    HIPCHK(c, hipMalloc((void**)&c->gabor2, P * 12));
    for (FrameSlot& f : c->slots) {
        HIPCHK(c, hipMalloc((void**)&f.tr1, P0 * 3 + 16)); HIPCHK(c, hipMalloc((void**)&f.tr2, P0 * 3 + 16));
        HIPCHK(c, hipMalloc((void**)&f.out, P * 3 + 16));
        HIPCHK(c, hipMalloc((void**)&f.triMap, P * 4));
        f.map_tag = 0;
        HIPCHK(c, hipMalloc((void**)&f.pyrL, off3 * 4)); HIPCHK(c, hipMalloc((void**)&f.pyrR, off3 * 4));
        HIPCHK(c, hipMalloc((void**)&f.pyrB, off3 * 4)); HIPCHK(c, hipMalloc((void**)&f.pyrM, off1 * 4));
        if (W < 2 || H < 2) { HIPCHK(c, hipMalloc((void**)&f.tmp, P * 12)); HIPCHK(c, hipMalloc((void**)&f.diff, P * 12)); }
    }
    if (c->use_tail) {
        HIPCHK(c, hipMalloc(&c->d_levels, c->tail.desc.size() * 4 + 16));
        if (!c->tail.desc.empty()) HIPCHK(c, hipMemcpy(c->d_levels, c->tail.desc.data(), c->tail.desc.size() * 4, hipMemcpyHostToDevice));
    }
    c->W = W; c->H = H;
    return alloc_slot_format(c);
}

int set_points(poppy_hip_ctx* c, const float* p1, const float* p2, int n) {
    if (n < 0 || (n > 0 && (!p1 || !p2))) return fail(c, POPPY_E_ARG, "bad point sets");
    c->fundamental.valid = false;                                  // (the set-up with the RANSAC filter sets it again behind this call)
    c->pts1_0.resize(n); c->pts2.resize(n);
    if (n) { memcpy(c->pts1_0.data(), p1, (size_t)n * 8); memcpy(c->pts2.data(), p2, (size_t)n * 8); }
    c->pts1 = c->pts1_0;
    const int rc = ensure_ring(c, n);
    if (rc == POPPY_OK) start_default_seq_plans(c);                // (the previous pair's plans, if a call never took them, are dropped in there)
    return rc;
}

int finish_pair_load(poppy_hip_ctx* c) {
    launch_gray_inv(c->gabor2, c->m2, c->W * c->H, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->inputs_ready, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));       // frames on other streams do not wait for the pair on the device: it is complete here
    c->cur1 = c->c1; c->cur1_ready = nullptr; c->last_slot = -1; c->pair_ready = true;
    return POPPY_OK;
}

// every frame queued on this context has finished (independent frames run on their slots' streams)
int drain_frames(poppy_hip_ctx* c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (FrameSlot& f : c->slots) {
        if (f.stream) HIPCHK(c, hipStreamSynchronize(f.stream));
        if (f.own_stream && f.own_stream != f.stream) HIPCHK(c, hipStreamSynchronize(f.own_stream));
        if (f.fmt.fmt_stream) HIPCHK(c, hipStreamSynchronize(f.fmt.fmt_stream));
    }
    return POPPY_OK;
}

int stage_pair_state(poppy_hip_ctx* c) {
    const int n = (int)c->pts1_0.size();
    if (n > kPairMaxPoints) return fail(c, POPPY_E_UNSUPPORTED, "more point pairs than the packed pair state has room for");
    std::vector<uint8_t> head(kPairHeadBytes + 2 * (size_t)kPairMaxPoints * 8, 0);
    PairStateHeader h{};
    h.magic = kPairMagic; h.version = 1; h.W = c->W; h.H = c->H; h.n_points = n; h.nfeatures = c->last_nfeatures;
    h.initial_morph_dist = c->initial_morph_dist; h.detail[0] = c->last_detail[0]; h.detail[1] = c->last_detail[1];
    memcpy(head.data(), &h, sizeof h);
    if (n) {
        memcpy(head.data() + kPairHeadBytes, c->pts1_0.data(), (size_t)n * 8);
        memcpy(head.data() + kPairHeadBytes + (size_t)kPairMaxPoints * 8, c->pts2.data(), (size_t)n * 8);
    }
    HIPCHK(c, hipMemcpyAsync(c->arena, head.data(), head.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));           // `head` goes out of scope
    return POPPY_OK;
}

int adopt_pair_state(poppy_hip_ctx* c) {
    std::vector<uint8_t> head(kPairHeadBytes + 2 * (size_t)kPairMaxPoints * 8);
    HIPCHK(c, hipMemcpyAsync(head.data(), c->arena, head.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    PairStateHeader h;
    memcpy(&h, head.data(), sizeof h);
    if (h.magic != kPairMagic || h.version != 1) return fail(c, POPPY_E_ARG, "not a packed pair state");
    if (h.W != c->W || h.H != c->H) return fail(c, POPPY_E_ARG, "packed pair state has another geometry");
    if (h.n_points < 0 || h.n_points > kPairMaxPoints) return fail(c, POPPY_E_ARG, "packed pair state is corrupt");
    c->last_nfeatures = h.nfeatures; c->initial_morph_dist = h.initial_morph_dist;
    c->last_detail[0] = h.detail[0]; c->last_detail[1] = h.detail[1];
    int rc = set_points(c, (const float*)(head.data() + kPairHeadBytes), (const float*)(head.data() + kPairHeadBytes + (size_t)kPairMaxPoints * 8), h.n_points);
    if (rc) return rc;
    c->c2_raw_valid = false;
    HIPCHK(c, hipEventRecord(c->inputs_ready, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));       // frames on other streams do not wait for the pair on the device: it is complete here
    c->cur1 = c->c1; c->cur1_ready = nullptr; c->last_slot = -1; c->pair_ready = true;
    return POPPY_OK;
}

int upload_image(poppy_hip_ctx* c, uint8_t* dst, const uint8_t* src, size_t stride, int W, int H) {
    // (tight rows go as one linear copy: kernels.h copy_rows_async; only images that really have padded rows — ROIs — pay the 2-D copy's slow path at odd widths)
    HIPCHK(c, copy_rows_async(dst, (size_t)W * 3, src, stride, (size_t)W * 3, H, hipMemcpyHostToDevice, c->stream));
    return POPPY_OK;
}

extern "C" {

int poppy_hip_pair_load(poppy_hip_ctx* c, const uint8_t* c1, size_t s1, const uint8_t* c2, size_t s2, const float* gabor2,
                        int W, int H, const float* p1, const float* p2, int n) {
    if (!c) return POPPY_E_ARG;
    if (!c1 || !c2 || !gabor2 || W <= 0 || H <= 0 || s1 < (size_t)W * 3 || s2 < (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad image arguments");
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    int rc = alloc_pair(c, W, H); if (rc) return rc;
    c->c2_raw_valid = false;
    rc = set_points(c, p1, p2, n); if (rc) return rc;
    rc = upload_image(c, c->c1, c1, s1, W, H); if (rc) return rc;
    rc = upload_image(c, c->c2, c2, s2, W, H); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->gabor2, gabor2, (size_t)W * H * 12, hipMemcpyHostToDevice, c->stream));
    rc = finish_pair_load(c); if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));      // host buffers may be reused by the caller
    return POPPY_OK;
}

int poppy_hip_pair_load_device(poppy_hip_ctx* c, const void* d1, const void* d2, const void* dg, int W, int H,
                               const float* p1, const float* p2, int n) {
    if (!c) return POPPY_E_ARG;
    if (!d1 || !d2 || !dg || W <= 0 || H <= 0) return fail(c, POPPY_E_ARG, "bad image arguments");
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    int rc = alloc_pair(c, W, H); if (rc) return rc;
    c->c2_raw_valid = false;
    rc = set_points(c, p1, p2, n); if (rc) return rc;
    const size_t P = (size_t)W * H;
    HIPCHK(c, hipMemcpyAsync(c->c1, d1, P * 3, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->c2, d2, P * 3, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->gabor2, dg, P * 12, hipMemcpyDeviceToDevice, c->stream));
    rc = finish_pair_load(c); if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return POPPY_OK;
}

int poppy_hip_pair_reset(poppy_hip_ctx* c) {
    if (!c) return POPPY_E_ARG;
    if (!c->pair_ready) return fail(c, POPPY_E_STATE, "no pair loaded");
    c->cur1 = c->c1; c->cur1_ready = nullptr; c->pts1 = c->pts1_0; c->last_slot = -1;
    return POPPY_OK;
}

int poppy_hip_render(poppy_hip_ctx* c, double shape, double mask, int chain, uint8_t* dst, size_t dst_stride) {
    if (!c) return POPPY_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = render_frame(c, shape, mask, chain != 0); if (rc) return rc;
    if (dst) {
        if (dst_stride < (size_t)c->W * 3) return fail(c, POPPY_E_ARG, "dst_stride too small");
        FrameSlot& f = c->slots[c->last_slot];
        hipStream_t fs = f.last_stream ? f.last_stream : c->stream;               // in order behind the frame itself
        HIPCHK(c, copy_rows_async(dst, dst_stride, f.out, (size_t)c->W * 3, (size_t)c->W * 3, c->H, hipMemcpyDeviceToHost, fs));
        HIPCHK(c, hipStreamSynchronize(fs));
    }
    return POPPY_OK;
}

const void* poppy_hip_frame_device(poppy_hip_ctx* c) { return (c && c->last_slot >= 0) ? c->slots[c->last_slot].out : nullptr; }
void* poppy_hip_frame_stream(poppy_hip_ctx* c) {
    if (!c || c->last_slot < 0) return nullptr;
    const FrameSlot& f = c->slots[c->last_slot];
    return (void*)(f.last_stream ? f.last_stream : c->stream);
}
int poppy_hip_frame_wait(poppy_hip_ctx* c, void* hip_stream) {
    if (!c) return POPPY_E_ARG;
    if (c->last_slot < 0) return fail(c, POPPY_E_STATE, "no frame rendered");
    HIPCHK(c, hipSetDevice(c->device));
    FrameSlot& f = c->slots[c->last_slot];
    if (hip_stream) HIPCHK(c, hipStreamWaitEvent((hipStream_t)hip_stream, f.done, 0));
    else HIPCHK(c, hipEventSynchronize(f.done));
    return POPPY_OK;
}

int poppy_hip_morph_images(poppy_hip_ctx* c, const uint8_t* c1, size_t s1, const uint8_t* c2, size_t s2, const float* gabor2, int W, int H,
                           const float* p1, const float* p2, int n, double shape, double mask, uint8_t* dst, size_t dst_stride, float* morphed) {
    if (!c) return POPPY_E_ARG;
    if (!dst) return fail(c, POPPY_E_ARG, "dst is null");
    int rc = poppy_hip_pair_load(c, c1, s1, c2, s2, gabor2, W, H, p1, p2, n); if (rc) return rc;
    rc = poppy_hip_render(c, shape, mask, 0, dst, dst_stride); if (rc) return rc;
    if (morphed && n) memcpy(morphed, c->plan.morphed.data(), (size_t)n * 8);
    return POPPY_OK;
}

double poppy_frame_ratio(int j, int number_of_frames, double phase) {
    const double N = (double)number_of_frames;
    const double linear = j / N;
    double progress = 0;
    if (phase >= 1.0) progress = 1;
    if (phase < 1.0 && phase >= 0) progress = 1.0 / N;
    else if (linear == 0) progress = 0;
    else if (linear == 1) progress = 1;
    else progress = (1.0 / (1.0 - linear)) / N;
    double shape = (phase < 1.0 && phase >= 0) ? progress * phase : progress;
    if (shape > 1) shape = 1;
    return shape;
}

int poppy_hip_morph_frames(poppy_hip_ctx* c, double phase, poppy_write_cb write, void* user) {
    if (!c) return POPPY_E_ARG;
    if (!c->pair_ready) return fail(c, POPPY_E_STATE, "no pair loaded");
    HIPCHK(c, hipSetDevice(c->device));
    const int N = c->cfg.number_of_frames;
    if (phase == 0 || phase == 1) {                            // src/poppy.hpp:54-70: N copies of image 1 / image 2, nothing rendered
        if (!write) return POPPY_OK;
        return write_device_image(c, phase == 0 ? c->c1 : (c->c2_raw_valid ? c->c2_raw : c->c2), c->W, c->H, N, write, user);
    }
    const int n = phase >= 0 ? 1 : N;                          // phase mode: exactly one frame (src/poppy.hpp:234-235)
    std::vector<double> ratio(n);
    for (int j = 0; j < n; ++j) ratio[j] = poppy_frame_ratio(j, N, phase);
    return render_sequence(c, ratio.data(), ratio.data(), n, true, write, user);
}

int poppy_hip_render_phases(poppy_hip_ctx* c, const double* t, int n, poppy_write_cb write, void* user) {
    if (!c || (n > 0 && !t) || n < 0) return POPPY_E_ARG;
    if (!c->pair_ready) return fail(c, POPPY_E_STATE, "no pair loaded");
    HIPCHK(c, hipSetDevice(c->device));
    // PAL8_SEQ: the call's frames, copies included, are one sequence: collected on the device, handed over at the end
    const bool seq = n > 0 && writer_wants_sequence(c, write != nullptr);
    if (seq) { int rc = seq_begin(c, n); if (rc) return rc; }
    for (int i = 0; i < n;) {
        int rc = POPPY_OK, j = i + 1;
        if (t[i] == 0 || t[i] == 1) {                             // a plain copy of image 1 / image 2
            const uint8_t* img = t[i] == 0 ? c->c1 : (c->c2_raw_valid ? c->c2_raw : c->c2);
            if (seq) rc = seq_add_image(c, img);
            else if (write) rc = write_device_image(c, img, c->W, c->H, 1, write, user);
        } else {
            while (j < n && t[j] != 0 && t[j] != 1) ++j;
            rc = poppy_hip_pair_reset(c);
            if (rc == POPPY_OK) rc = render_sequence(c, t + i, t + i, j - i, false, write, user, seq);
        }
        if (rc) { if (seq) seq_abort_keep_error(c); return rc; }
        i = j;
    }
    return seq ? seq_finish(c, write, user) : POPPY_OK;
}

int poppy_printed_morph_distance(const float* p1, const float* p2, int n, int W, int H, double* out) {
    if (n < 1 || !p1 || !p2 || !out || W <= 0 || H <= 0) return POPPY_E_ARG;
    std::vector<P2f> a(n), b(n), u1, u2;
    memcpy(a.data(), p1, (size_t)n * 8); memcpy(b.data(), p2, (size_t)n * 8);
    clip_points_ref(a, W, H); unique_points_ref(a, u1);           // src/poppy.hpp:142-157
    clip_points_ref(b, W, H); unique_points_ref(b, u2);
    if (u1.size() > u2.size()) u1.resize(u2.size()); else u2.resize(u1.size());
    *out = morph_distance_ref(u1, u2, W, H);
    return POPPY_OK;
}

int poppy_hip_pair_distance(poppy_hip_ctx* c, double* out) {
    if (!c || !out) return POPPY_E_ARG;
    if (!c->pair_ready) return fail(c, POPPY_E_STATE, "no pair loaded");
    if (c->pts1_0.empty()) return fail(c, POPPY_E_NOMATCH, "no point pairs");
    return poppy_printed_morph_distance((const float*)c->pts1_0.data(), (const float*)c->pts2.data(), (int)c->pts1_0.size(), c->W, c->H, out);
}

long poppy_hypotf_selfcheck(long n, uint64_t seed) { return hypotf_selfcheck(n, seed); }

int poppy_hip_morph(poppy_hip_ctx* c, const uint8_t* bgr1, size_t s1, const uint8_t* bgr2, size_t s2, int W, int H, double phase,
                    int distance, poppy_write_cb write, void* user, double* morph_distance) {
    if (!c) return POPPY_E_ARG;
    if (!bgr1 || !bgr2 || W <= 0 || H <= 0 || s1 < (size_t)W * 3 || s2 < (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad image arguments");
    const int N = c->cfg.number_of_frames;
    if (phase == 0 || phase == 1)                              // src/poppy.hpp:54-70, before any feature work (converted on the host, no GPU touched)
        return write && N > 0 ? write_host_image(c, phase == 0 ? bgr1 : bgr2, phase == 0 ? s1 : s2, W, H, N, write, user) : POPPY_OK;
    int rc = poppy_hip_pair_begin(c, bgr1, s1, bgr2, s2, W, H); if (rc) return rc;
    if (c->pts1_0.empty()) {                                   // :125-134 (see the header: the reference throws before reaching it)
        if (!distance && write) {
            std::vector<uint8_t> blend((size_t)W * 3 * H);
            rc = poppy_hip_dissolve(c, bgr1, s1, bgr2, s2, W, H, phase, blend.data(), (size_t)W * 3); if (rc) return rc;
            rc = write_device_image(c, c->slots[0].out, W, H, N, write, user); if (rc) return rc;      // the blend, still in slot 0
        }
        return fail(c, POPPY_E_NOMATCH, "no point pairs: linear-blend fallback frames written (src/poppy.hpp:125-134)");
    }
    if (morph_distance || distance) {
        double d = 0;
        rc = poppy_hip_pair_distance(c, &d); if (rc) return rc;
        if (morph_distance) *morph_distance = d;
    }
    if (distance) return POPPY_OK;                             // :159-163 (the reference exits here)
    return poppy_hip_morph_frames(c, phase, write, user);
}

int poppy_hip_dissolve(poppy_hip_ctx* c, const uint8_t* img1, size_t s1, const uint8_t* img2, size_t s2, int W, int H, double phase,
                       uint8_t* dst, size_t dst_stride) {
    if (!c) return POPPY_E_ARG;
    if (!img1 || !img2 || !dst || W <= 0 || H <= 0) return fail(c, POPPY_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    int rc = alloc_pair(c, W, H); if (rc) return rc;
    rc = upload_image(c, c->c1, img1, s1, W, H); if (rc) return rc;
    rc = upload_image(c, c->c2, img2, s2, W, H); if (rc) return rc;
    // Mat blend = img2*phase + img1*(1.0-phase)  ->  addWeighted(img2, phase, img1, 1-phase, 0)
    launch_dissolve(c->c2, c->c1, c->slots[0].out, (size_t)W * H * 3, (float)phase, (float)(1.0 - phase), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, copy_rows_async(dst, dst_stride, c->slots[0].out, (size_t)W * 3, (size_t)W * 3, H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pair_ready = false;
    return POPPY_OK;
}

int poppy_hip_debug_fetch(poppy_hip_ctx* c, const char* name, void* host, size_t bytes) {
    if (!c || !name || !host) return POPPY_E_ARG;
    if (!c->W) return fail(c, POPPY_E_STATE, "no pair loaded");
    const size_t P = (size_t)c->W * c->H;
    const void* src = nullptr; size_t need = 0;
    size_t px_bytes = 0;                          // set for the buffers whose rows may be padded (level 0 of the slot's own images): bytes per pixel
    std::string n(name);
    if (n != "m2" && n != "gabor2" && c->last_slot < 0) return fail(c, POPPY_E_STATE, "no frame rendered yet");
    const FrameSlot& f = c->slots[c->last_slot < 0 ? 0 : c->last_slot];          // intermediates of the last frame
    if (n == "triMap") { src = f.triMap; need = P * 4; }
    else if (n == "trImg1") { src = f.tr1; need = P * 3; px_bytes = 3; }
    else if (n == "trImg2") { src = f.tr2; need = P * 3; px_bytes = 3; }
    else if (n == "lbmask") {
        if (c->lazy_mask) {                    // never materialised by the frame: made here from m2 and the frame's (alpha, beta)
            if (hipStreamSynchronize(f.last_stream ? f.last_stream : c->stream) != hipSuccess) return fail(c, POPPY_E_DEVICE, "sync failed");
            launch_lbmask(c->m2, (const double*)(f.d_blob + kBlobMaskAB), f.pyrM, P, c->stream);
            if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, POPPY_E_DEVICE, "lbmask kernel failed");
        }
        src = f.pyrM; need = P * 4; px_bytes = 4;
    }
    else if (n == "lapBlend") { src = f.pyrB; need = P * 12; px_bytes = 12; }
    else if (n == "unsharp") {
        if (!c->debug || !f.unsharpF) return fail(c, POPPY_E_STATE, "enable debug before rendering the frame");
        src = f.unsharpF; need = P * 12;
    }
    else if (n == "m2") { src = c->m2; need = P * 4; }
    else if (n == "gabor2") { src = c->gabor2; need = P * 12; }
    else return fail(c, POPPY_E_ARG, "unknown debug buffer");
    if (bytes != need) return fail(c, POPPY_E_ARG, "debug buffer size mismatch");
    { int rc = drain_frames(c); if (rc) return rc; }
    if (px_bytes && c->levels[0].pitch != c->W)
        HIPCHK(c, hipMemcpy2D(host, (size_t)c->W * px_bytes, src, (size_t)c->levels[0].pitch * px_bytes, (size_t)c->W * px_bytes, c->H, hipMemcpyDeviceToHost));
    else HIPCHK(c, hipMemcpy(host, src, need, hipMemcpyDeviceToHost));
    return POPPY_OK;
}

int poppy_hip_debug_triangles(poppy_hip_ctx* c, int* n_tris, int* idx3, float* M1, float* M2, int max_tris) {
    if (!c || !n_tris) return POPPY_E_ARG;
    const int T = c->plan.n_tris;
    *n_tris = T;
    if (T > max_tris) return fail(c, POPPY_E_ARG, "max_tris too small");
    if (idx3 && T) memcpy(idx3, c->plan.idx3.data(), (size_t)T * 3 * sizeof(int));
    if (M1 && T) memcpy(M1, c->plan.M1.data(), (size_t)T * 9 * sizeof(float));
    if (M2 && T) memcpy(M2, c->plan.M2.data(), (size_t)T * 9 * sizeof(float));
    return POPPY_OK;
}

int poppy_plan_frame(int W, int H, const float* p1, const float* p2, int n, double shape, int max_tris,
                     int* n_tris, int* idx3, int* tri_xy, float* M1, float* M2, float* inv1, float* inv2, float* morphed) {
    if (W <= 0 || H <= 0 || n < 0 || !n_tris) return POPPY_E_ARG;
    std::vector<P2f> a(n), b(n);
    if (n) { memcpy(a.data(), p1, (size_t)n * 8); memcpy(b.data(), p2, (size_t)n * 8); }
    FramePlan plan;
    if (plan_frame(W, H, a, b, shape, plan)) return POPPY_E_RANGE;
    const int T = plan.n_tris;
    *n_tris = T;
    if (T > max_tris) return POPPY_E_ARG;
    if (idx3 && T) memcpy(idx3, plan.idx3.data(), (size_t)T * 12);
    if (tri_xy && T) memcpy(tri_xy, plan.tri_xy.data(), (size_t)T * 24);
    if (M1 && T) memcpy(M1, plan.M1.data(), (size_t)T * 36);
    if (M2 && T) memcpy(M2, plan.M2.data(), (size_t)T * 36);
    if (inv1 && T) memcpy(inv1, plan.inv1.data(), (size_t)T * 36);
    if (inv2 && T) memcpy(inv2, plan.inv2.data(), (size_t)T * 36);
    if (morphed && n) memcpy(morphed, plan.morphed.data(), (size_t)n * 8);
    return POPPY_OK;
}

// the frame's plan binned as a context would bin it for n point pairs; *ok = the lists fit its room (they are built in full either way)
static int plan_tile_bins(int W, int H, const float* p1, const float* p2, int n, double shape, int tile_w, FramePlan& plan, bool* ok) {
    if (W <= 0 || H <= 0 || n < 0 || (n > 0 && (!p1 || !p2)) || (tile_w != 64 && tile_w != 128)) return POPPY_E_ARG;
    std::vector<P2f> a(n), b(n);
    if (n) { memcpy(a.data(), p1, (size_t)n * 8); memcpy(b.data(), p2, (size_t)n * 8); }
    if (plan_frame(W, H, a, b, shape, plan)) return POPPY_E_RANGE;
    *ok = build_tile_bins(plan, W, H, tile_w, 1024 / tile_w, tile_bins_capacity(n, W, H, tile_w));
    if (!*ok && !build_tile_bins(plan, W, H, tile_w, 1024 / tile_w, SIZE_MAX)) return POPPY_E_UNSUPPORTED;     // the lists a context would have needed room for
    return POPPY_OK;
}

int poppy_plan_tile_counts(int W, int H, const float* p1, const float* p2, int n, double shape, int tile_w,
                           int* counts, int cap, int* n_tiles, long long* total, int* bins_ok) {
    if (!n_tiles) return POPPY_E_ARG;
    FramePlan plan;
    bool ok = false;
    if (int rc = plan_tile_bins(W, H, p1, p2, n, shape, tile_w, plan, &ok)) return rc;
    const int nt = (int)plan.tile_off.size() - 1;
    *n_tiles = nt;
    if (total) *total = (long long)plan.tile_tris.size();
    if (bins_ok) *bins_ok = ok;
    if (!counts) return POPPY_OK;
    if (nt > cap) return POPPY_E_ARG;
    for (int i = 0; i < nt; ++i) counts[i] = plan.tile_off[i + 1] - plan.tile_off[i];
    return POPPY_OK;
}

int poppy_plan_blob_layout(int capacity, int n_tris, long long n_work, long long n_toff, long long n_ttri, int fused, unsigned long long* out) {
    if (!out || n_tris < 0 || n_work < 0 || n_toff < 0 || n_ttri < 0) return POPPY_E_ARG;
    if (capacity) {                                            // (n_points, W, H, tile width) -> what ensure_ring allocates a slot's blob with
        const int n_points = n_tris, W = (int)n_work, H = (int)n_toff;
        if (W <= 0 || H <= 0 || n_work > 16384 || n_toff > 16384 || (n_ttri != 0 && n_ttri != 64 && n_ttri != 128)) return POPPY_E_ARG;
        const int need = plan_triangle_budget(n_points), tw = n_ttri ? (int)n_ttri : warp_bin_tile_width(W, H);
        const size_t ntiles = tile_count(W, H, tw), bins_cap = tile_bins_capacity(n_points, W, H, tw);
        const unsigned long long v[9] = {plan_blob_capacity(need, H, ntiles, bins_cap), (unsigned long long)need, ntiles, bins_cap, (unsigned long long)tw, 0, 0, 0, 0};
        memcpy(out, v, sizeof v);
        return POPPY_OK;
    }
    const PlanBlobLayout l = plan_blob_layout(n_tris, (size_t)n_work, (size_t)n_toff, (size_t)n_ttri, fused != 0);
    const unsigned long long v[9] = {l.rec_bytes, l.o_edges, l.o_outl, l.o_toff, l.o_ttri, l.o_tri, l.o_inv, l.o_work, l.used};
    memcpy(out, v, sizeof v);
    return POPPY_OK;
}

int poppy_plan_tile_tris(int W, int H, const float* p1, const float* p2, int n, double shape, int tile_w,
                         int* tris, long long cap, long long* total) {
    if (!total) return POPPY_E_ARG;
    FramePlan plan;
    bool ok = false;
    if (int rc = plan_tile_bins(W, H, p1, p2, n, shape, tile_w, plan, &ok)) return rc;
    *total = (long long)plan.tile_tris.size();
    if (!tris) return POPPY_OK;
    if (*total > cap) return POPPY_E_ARG;
    for (size_t i = 0; i < plan.tile_tris.size(); ++i) tris[i] = plan.tile_tris[i];
    return POPPY_OK;
}

int poppy_hip_pair_points(poppy_hip_ctx* c, float* p1, float* p2, int max_points, int* n_points) {
    if (!c || !n_points) return POPPY_E_ARG;
    const int n = (int)c->pts1_0.size();
    *n_points = n;
    if (n > max_points) return fail(c, POPPY_E_ARG, "max_points too small");
    if (p1 && n) memcpy(p1, c->pts1_0.data(), (size_t)n * 8);
    if (p2 && n) memcpy(p2, c->pts2.data(), (size_t)n * 8);
    return POPPY_OK;
}

int poppy_hip_timing_summary(poppy_hip_ctx* c, const char** names, float* total_ms, int* launches, int max) {
    if (!c) return 0;
    if (drain_frames(c) != POPPY_OK) return 0;
    int n = 0;
    for (size_t i = 1; i < c->marks_used; ++i) {
        const char* nm = c->marks[i].name;
        if (!nm) continue;                                  // frame boundary
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->marks[i - 1].ev, c->marks[i].ev) != hipSuccess) continue;
        int k = 0;
        while (k < n && strcmp(names[k], nm) != 0) ++k;
        if (k == n) { if (n >= max) continue; names[n] = nm; total_ms[n] = 0.f; launches[n] = 0; ++n; }
        total_ms[k] += ms; launches[k] += 1;
    }
    c->marks_used = 0;
    return n;
}

int poppy_hip_render_many(poppy_hip_ctx* c, const double* shape, const double* mask, int n, int chain, poppy_write_cb write, void* user) {
    if (!c || !shape || !mask || n < 0) return POPPY_E_ARG;
    if (!c->pair_ready) return fail(c, POPPY_E_STATE, "no pair loaded");
    HIPCHK(c, hipSetDevice(c->device));
    return render_sequence(c, shape, mask, n, chain != 0, write, user);
}

}  // extern "C"
