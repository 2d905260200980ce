// palette_seq.cpp — the POPPY_FRAME_PAL8_SEQ / POPPY_FRAME_GIF_SEQ sequence (palette_seq.h): collecting a call's frames in the store, the palette, the two hand-over
// loops through the writer ring, and the call-scoped sequence of poppy_hip_bgr_frames_to_gif_frames.
#include "context.h"

int seq_begin(poppy_hip_ctx* c, int n) {
    const WriterGeom g = writer_geom(c);
    const int W = g.w, H = g.h;
    PaletteSeq& q = c->seq;
    if (q.open) { int rc = seq_abort(c); if (rc) return rc; }      // (a sequence that a device error left open: its frames and sums are dropped, not mixed into this one)
    if (const char* why = sequence_refuses(c->frame_format, n, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);      // (a sequence format: writer_wants_sequence)
    { int rc = alloc_slot_format(c); if (rc) return rc; }
    const size_t stride = ((size_t)W * H * 3 + 15) & ~(size_t)15, need = stride * (size_t)n;      // (every frame's place begins on a 16-byte boundary)
    if (q.store.reserve(need) != hipSuccess) { (void)hipGetLastError(); return fail(c, POPPY_E_DEVICE, "no device memory for the sequence's frames (3 * width * height bytes each)"); }
    q.stride = stride; q.n = n; q.count = 0; q.open = true;
    return POPPY_OK;
}

bool seq_wanted(const poppy_hip_ctx* c) { return c->seq.open && writer_wants_sequence(c, c->writer_attached); }
int seq_pass(poppy_hip_ctx* c, const uint8_t* d_bgr, uint8_t* dst, hipStream_t s, hipEvent_t done) {
    const WriterGeom g = writer_geom(c);
    launch_pal8_seq_pass(d_bgr, dst, c->seq.tables, g.w, g.h, s, done);
    HIPCHK(c, hipGetLastError());
    return POPPY_OK;
}
uint8_t* seq_next_place(poppy_hip_ctx* c) { return c->seq.count < c->seq.n ? c->seq.store.p + (size_t)c->seq.count++ * c->seq.stride : nullptr; }

int seq_add_image(poppy_hip_ctx* c, const uint8_t* d_bgr) {
    uint8_t* dst = seq_next_place(c);
    if (!dst) return fail(c, POPPY_E_STATE, "more frames than the sequence was opened for");
    Timer tm(c, c->stream);
    if (c->timing == 1) tm.mark(nullptr);
    const WriterGeom g = writer_geom(c);
    if (g.scaled()) {
        int rc = scale_into_scratch(c, d_bgr, c->W, c->H, g); if (rc) return rc;
        if (c->timing == 1) tm.mark(scaling_mark(g));
        d_bgr = c->scale_scratch.p;
    }
    { int rc = seq_pass(c, d_bgr, dst, c->stream, nullptr); if (rc) return rc; }
    if (c->timing == 1) tm.mark("pal8_seq_hist");
    return POPPY_OK;
}

int seq_abort(poppy_hip_ctx* c) {
    c->seq.open = false;
    int rc = drain_frames(c);
    if (c->seq.tables && hipMemset(c->seq.tables, 0, kPal8SeqTableOffset) != hipSuccess && rc == POPPY_OK) rc = fail(c, POPPY_E_DEVICE, "could not clear the sequence tables");
    return rc;
}
void seq_abort_keep_error(poppy_hip_ctx* c) { const std::string why = c->err; (void)seq_abort(c); c->err = why; }

// Every frame as PAL8_SEQ: the index plane from the store through a ring of R device planes and R pinned buffers, remap and copy in order on the ring buffer's own
// stream (render_sequence_frames: no event behind a copy), the palette behind the indices on the host.
static int seq_hand_over_indices(poppy_hip_ctx* c, poppy_write_cb write, void* user) {
    PaletteSeq& q = c->seq;
    const WriterGeom g = writer_geom(c);
    const int n = q.count, W = g.w, H = g.h;
    const bool marks = c->timing == 1;
    uint8_t pal[768];
    HIPCHK(c, hipMemcpyAsync(pal, q.tables + kPal8SeqPaletteOffset, 768, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t n_px = (size_t)W * H, plane = (n_px + 255) & ~(size_t)255;
    WriterRing ring;
    { int rc = ring.open(c, n_px + 768, false); if (rc) return rc; }
    HIPCHK(c, q.idx.reserve(plane * ring.R));
    auto deliver = [&]() -> int {
        uint8_t* frame = nullptr;
        HIPCHK(c, ring.deliver_next(c, false, &frame));
        memcpy(frame + n_px, pal, 768);
        write(user, frame, W, H, writer_stride(POPPY_FRAME_PAL8_SEQ, W));
        return POPPY_OK;
    };
    for (; ring.issued < n; ++ring.issued) {
        const int k = ring.issued;
        if (k >= ring.R) { int rc = deliver(); if (rc) return rc; }
        hipStream_t s = nullptr;
        HIPCHK(c, ring.stream(c, k, &s));
        uint8_t* d_idx = q.idx.p + (size_t)(k % ring.R) * plane;
        Timer tm(c, s);
        if (marks) tm.mark(nullptr);
        launch_pal8_seq_remap(q.store.p + (size_t)k * q.stride, q.tables, d_idx, W, H, s);
        if (marks) tm.mark("frame_format");
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(ring.buffer(k), d_idx, n_px, hipMemcpyDeviceToHost, s));
    }
    while (ring.written < n) { int rc = deliver(); if (rc) return rc; }
    return POPPY_OK;
}

// the coding pair of one frame of a sequence: from its BGR (its place in a sequence store) through seq_tables, into `frame`; the length also into total_dev (null: none)
static void enqueue_seq_gif_coding(const uint8_t* bgr, const uint8_t* seq_tables, uint8_t* scratch, uint8_t* frame, void* total_dev, int W, int H, hipStream_t s, Timer* tm) {
    launch_gif_lzw_bgr(bgr, seq_tables, scratch, W, H, s);
    if (tm) tm->mark("gif_lzw");
    launch_gif_pack_seq(seq_tables, scratch, frame, (uint32_t*)total_dev, W, H, s);
    if (tm) tm->mark("gif_pack");
}

// Every frame as GIF_SEQ: coded from its place in the store (k_gif_lzw_bgr: no index plane) into one of R device buffers, each followed by the coder's scratch, on the
// ring buffer's own stream; k_gif_pack stores the frame's length into the ring buffer's pinned word.  The host waits for that stream, reads the word, bounds-checks it
// as slot_frame_length does and queues the copy of exactly that many bytes on the same stream — no event behind a copy.  Frame k + 1 is being coded (on the next ring
// buffer's stream) while the host waits for frame k's length, its copy runs and the writer has the frames before it; the writer gets the frames in order.
static int seq_hand_over_coded(poppy_hip_ctx* c, poppy_write_cb write, void* user) {
    PaletteSeq& q = c->seq;
    const WriterGeom g = writer_geom(c);
    const int n = q.count, W = g.w, H = g.h;
    const bool marks = c->timing == 1;
    const size_t capacity = poppy_frame_bytes(POPPY_FRAME_GIF_SEQ, W, H), frame_part = (capacity + 16 + 255) & ~(size_t)255;
    const size_t each = frame_part + ((gif_scratch_bytes(W, H) + 255) & ~(size_t)255);
    WriterRing ring;
    { int rc = ring.open(c, capacity, false); if (rc) return rc; }
    HIPCHK(c, q.gif.reserve(each * ring.R));
    if (!q.gif_total) {
        HIPCHK(c, hipHostMalloc((void**)&q.gif_total, 64 * poppy_hip_ctx::kStageRing, hipHostMallocMapped));
        HIPCHK(c, hipHostGetDevicePointer((void**)&q.gif_total_dev, q.gif_total, 0));
    }
    auto d_frame = [&](int k) { return q.gif.p + (size_t)(k % ring.R) * each; };
    auto total_word = [&](int k) { return (volatile uint32_t*)((uint8_t*)q.gif_total + 64 * (size_t)(k % ring.R)); };
#ifdef POPPY_EXPERIMENTS
    const size_t plane = ((size_t)W * H + 255) & ~(size_t)255;
    HIPCHK(c, q.idx.reserve(plane * ring.R));
    const bool two_dispatch = getenv("POPPY_GIF_SEQ_TWO_DISPATCH") != nullptr;      // timing experiment, read per sequence so that one process alternates: the index plane through HBM (k_pal8_remap, then k_gif_lzw); the same bytes
#endif
    int coded = 0;                                                 // frames 0 .. coded - 1: their coding is queued; ring.issued: their copies are
    auto code_next = [&]() -> int {
        const int k = coded;
        hipStream_t s = nullptr;
        HIPCHK(c, ring.stream(c, k, &s));
        *total_word(k) = 0;                                        // (the buffer's last frame has been handed over: nothing writes the word now)
        Timer tm(c, s);
        if (marks) tm.mark(nullptr);
#ifdef POPPY_EXPERIMENTS
        if (two_dispatch) {
            uint8_t* d_idx = q.idx.p + (size_t)(k % ring.R) * plane;
            launch_pal8_seq_remap(q.store.p + (size_t)k * q.stride, q.tables, d_idx, W, H, s);
            if (marks) tm.mark("frame_format");
            launch_gif_lzw(d_idx, d_frame(k) + frame_part, W, H, s);
            if (marks) tm.mark("gif_lzw");
            launch_gif_pack_seq(q.tables, d_frame(k) + frame_part, d_frame(k), (uint32_t*)(q.gif_total_dev + 64 * (size_t)(k % ring.R)), W, H, s);
            if (marks) tm.mark("gif_pack");
        } else
#endif
        enqueue_seq_gif_coding(q.store.p + (size_t)k * q.stride, q.tables, d_frame(k) + frame_part, d_frame(k), q.gif_total_dev + 64 * (size_t)(k % ring.R), W, H, s, marks ? &tm : nullptr);
        HIPCHK(c, hipGetLastError());
        ++coded;
        return POPPY_OK;
    };
    auto copy_next = [&]() -> int {
        const int k = ring.issued;
        hipStream_t s = nullptr;
        HIPCHK(c, ring.stream(c, k, &s));
        HIPCHK(c, hipStreamSynchronize(s));                        // the frame is coded, its length is in the pinned word
        const size_t total = *total_word(k);
        if (!coded_length_ok(total, capacity, kGifFrameMinBytes)) return fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds");
        HIPCHK(c, hipMemcpyAsync(ring.buffer(k), d_frame(k), total, hipMemcpyDeviceToHost, s));
        ++ring.issued;
        return POPPY_OK;
    };
    auto deliver = [&]() -> int {
        if (ring.issued == ring.written) { int rc = copy_next(); if (rc) return rc; }
        uint8_t* frame = nullptr;
        HIPCHK(c, ring.deliver_next(c, false, &frame));
        write(user, frame, W, H, writer_stride(POPPY_FRAME_GIF_SEQ, W));
        return POPPY_OK;
    };
    int rc = POPPY_OK;
    while (coded < n && rc == POPPY_OK) {
        if (coded >= ring.R) rc = deliver();                       // frame coded - R has left its ring buffer, device and pinned
        if (rc == POPPY_OK) rc = code_next();
        if (rc == POPPY_OK && ring.issued < coded - 1) rc = copy_next();      // the frame before it, while this one is coded
    }
    while (ring.written < n && rc == POPPY_OK) rc = deliver();
    if (rc) for (int r = 0; r < ring.R; ++r) if (c->dl_ring[r]) (void)hipStreamSynchronize(c->dl_ring[r]);      // nothing writes the ring's buffers or words behind a failure
    return rc;
}

static int seq_hand_over(poppy_hip_ctx* c, poppy_write_cb write, void* user) {
    PaletteSeq& q = c->seq;
    q.open = false;
    { int rc = drain_frames(c); if (rc) return rc; }              // every pass has added its frame (they ran on the slots' streams)
    {
        Timer tm(c, c->stream);
        if (c->timing == 1) tm.mark(nullptr);
        launch_pal8_seq_build(q.tables, c->stream);
        if (c->timing == 1) tm.mark("pal8_seq_build");
    }
    HIPCHK(c, hipGetLastError());
    if (!format_traits(c->frame_format)->coded()) return seq_hand_over_indices(c, write, user);
    HIPCHK(c, hipStreamSynchronize(c->stream));                   // the ring's streams read the tables
    return seq_hand_over_coded(c, write, user);
}

int seq_finish(poppy_hip_ctx* c, poppy_write_cb write, void* user) {
    if (c->seq.count != c->seq.n) { (void)seq_abort(c); return fail(c, POPPY_E_STATE, "fewer frames than the sequence was opened for"); }
    const int rc = seq_hand_over(c, write, user);
    if (rc) seq_abort_keep_error(c);
    return rc;
}

extern "C" {

int poppy_hip_bgr_frames_to_gif_frames(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int W, int H, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    if (!bgr || !dst || W <= 0 || H <= 0 || stride < (size_t)W * 3 || n_frames < 1) return fail(c, POPPY_E_ARG, "bad arguments");
    if (const char* why = sequence_refuses(POPPY_FRAME_GIF_SEQ, n_frames, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    if (c->seq.open) return fail(c, POPPY_E_STATE, "a sequence is open on this context");
    HIPCHK(c, hipSetDevice(c->device));
    if (!prepare_pal8()) return fail(c, POPPY_E_DEVICE, "could not raise the palette build's LDS limit");
    // everything lives for the call: the context's own sequence tables, store and rings are not touched
    const size_t row = (size_t)W * 3, place = (row * H + 15) & ~(size_t)15, capacity = poppy_frame_bytes(POPPY_FRAME_GIF_SEQ, W, H);
    CallBuffers held;
    uint8_t *store = nullptr, *tables = nullptr, *work = nullptr, *frame = nullptr;
    hipError_t e = held.alloc(&store, place * (size_t)n_frames);
    if (e == hipSuccess) e = held.alloc(&tables, kPal8SeqTableBytes);
    if (e == hipSuccess) e = held.alloc(&work, gif_scratch_bytes(W, H));
    if (e == hipSuccess) e = held.alloc(&frame, capacity + 16);
    if (e == hipSuccess) e = hipMemsetAsync(tables, 0, kPal8SeqTableBytes, c->stream);
    for (int k = 0; k < n_frames && e == hipSuccess; ++k) {
        e = hipMemcpy2D(store + (size_t)k * place, row, bgr + (size_t)k * frame_stride, stride, row, (size_t)H, hipMemcpyHostToDevice);
        if (e == hipSuccess) { launch_pal8_seq_pass(store + (size_t)k * place, nullptr, tables, W, H, c->stream); e = hipGetLastError(); }
    }
    if (e == hipSuccess) { launch_pal8_seq_build(tables, c->stream); e = hipGetLastError(); }
    int rc = POPPY_OK;
    for (int k = 0; k < n_frames && e == hipSuccess && rc == POPPY_OK; ++k) {
        uint32_t total = 0;
        enqueue_seq_gif_coding(store + (size_t)k * place, tables, work, frame, nullptr, W, H, c->stream, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&total, frame, 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess && !coded_length_ok(total, capacity, kGifFrameMinBytes)) rc = fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds");
        else if (e == hipSuccess) e = hipMemcpy(dst + (size_t)k * capacity, frame, total, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(c->stream);   // nothing of the call is in flight when its buffers go (`held`, at the return)
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("GIF sequence coding: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return rc;
}

}  // extern "C"
