// palette_seq.cpp — the sequence formats (palette_seq.h: POPPY_FRAME_PAL8_SEQ / GIF_SEQ on one palette, POPPY_FRAME_JPEG_SEQ / JPEG444_SEQ on one table set,
// POPPY_FRAME_PNG_SEQ on one ninth table):
// collecting a call's frames in the store, the palette or the tables, the two hand-over loops through the writer ring, and the call-scoped sequences of
// poppy_hip_bgr_frames_to_gif_frames, poppy_hip_bgr_frames_to_jpeg_seq_frames and poppy_hip_bgr_frames_to_png_seq_frames.
#include "context.h"

// the context's sequence under a JPEG format: its record's sampling, its counts and its built tables (PaletteSeq::jpeg)
static bool seq_is_jpeg(const poppy_hip_ctx* c) { return format_traits(c->frame_format)->coder == kCoderJpeg; }
// ... under POPPY_FRAME_JPEG / JPEG444 with a sequence budget: no counts and no built tables, the sequence's search instead (PaletteSeq::budget)
static bool seq_is_budget(const poppy_hip_ctx* c) { const FormatTraits& t = writer_traits(c, c->frame_format); return t.coder == kCoderJpeg && !t.frame_tables; }
static uint32_t* seq_jpeg_counts(const PaletteSeq& q) { return (uint32_t*)q.jpeg; }
static const void* seq_jpeg_built(const PaletteSeq& q) { return q.jpeg + sizeof(jpeg::SymbolCounts); }
// ... under PNG: its sums and its built table (PaletteSeq::png)
static bool seq_is_png(const poppy_hip_ctx* c) { return format_traits(c->frame_format)->coder == kCoderPng; }
static uint32_t* seq_png_sums(const PaletteSeq& q) { return (uint32_t*)q.png; }
static void* seq_png_table(const PaletteSeq& q) { return q.png + kPngSeqSumWords * 4; }
// what waits in the store: the planes that a JPEG sequence's coder reads, the filtered stream in its coder's scratch under PNG, the BGR frame under a palette sequence
static size_t seq_held_bytes(const FormatTraits& t, int W, int H) {
    return t.coder == kCoderPng ? png_scratch_bytes(W, H, t.variant) : raster_bytes(t.coder == kCoderJpeg ? t.raster : kRasterNone, (size_t)W, (size_t)H);
}

int seq_begin(poppy_hip_ctx* c, int n) {
    const WriterGeom g = writer_geom(c);
    const int W = g.w, H = g.h;
    PaletteSeq& q = c->seq;
    if (q.open) { int rc = seq_abort(c); if (rc) return rc; }      // (a sequence that a device error left open: its frames and sums are dropped, not mixed into this one)
    if (const char* why = sequence_refuses(c->frame_format, n, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);      // (a sequence format: writer_wants_sequence)
    { int rc = alloc_slot_format(c); if (rc) return rc; }
    const FormatTraits& t = writer_traits(c, c->frame_format);
    const size_t stride = (seq_held_bytes(t, W, H) + 15) & ~(size_t)15, need = stride * (size_t)n;      // (every frame's place begins on a 16-byte boundary)
    if (seq_is_budget(c) && q.budget.reserve(jpeg_seq_budget_bytes(n, W, H, t.sampling())) != hipSuccess) { (void)hipGetLastError(); return fail(c, POPPY_E_DEVICE, "no device memory for the sequence budget's measured lengths (8 bytes per segment and frame)"); }
    if (q.store.reserve(need) != hipSuccess) { (void)hipGetLastError(); return fail(c, POPPY_E_DEVICE, "no device memory for the sequence's frames (3 * width * height bytes each, half of that as I420 planes, height more as PNG's filtered stream)"); }
    q.stride = stride; q.n = n; q.count = 0; q.open = true;
    return POPPY_OK;
}

bool seq_wanted(const poppy_hip_ctx* c) { return c->seq.open && writer_wants_sequence(c, c->writer_attached); }
int seq_pass(poppy_hip_ctx* c, const uint8_t* d_bgr, uint8_t* dst, hipStream_t s, hipEvent_t done) {
    const WriterGeom g = writer_geom(c);
    const FormatTraits& t = writer_traits(c, c->frame_format);
    if (t.coder == kCoderJpeg && !t.frame_tables)                  // under a sequence budget: the planes straight into the frame's place, nothing else (the mark behind it is frame_format)
        (t.raster == kRasterI444 ? launch_bgr_to_i444 : launch_bgr_to_i420)(d_bgr, dst, g.w, g.h, s, done);
    else if (t.coder == kCoderJpeg) {                              // the planes straight into the frame's place, then their symbols into the sequence's counts
        Timer tm(c, s);
        (t.raster == kRasterI444 ? launch_bgr_to_i444 : launch_bgr_to_i420)(d_bgr, dst, g.w, g.h, s, nullptr);
        if (c->timing == 1) tm.mark("frame_format");
        launch_jpeg_count_into(dst, c->jpeg_tables, seq_jpeg_counts(c->seq), g.w, g.h, t.sampling(), s, done);
    } else if (t.coder == kCoderPng) {                             // the filtered stream straight into the frame's place, then its tokens into the sequence's sums
        Timer tm(c, s);
        launch_png_filter(d_bgr, dst, g.w, g.h, t.variant, s);
        if (c->timing == 1) tm.mark("png_filter");
        launch_png_seq_count(dst, seq_png_sums(c->seq), g.w, g.h, s, done);
    } else launch_pal8_seq_pass(d_bgr, dst, c->seq.tables, g.w, g.h, s, done);
    HIPCHK(c, hipGetLastError());
    return POPPY_OK;
}
const char* seq_pass_mark(const poppy_hip_ctx* c) { return seq_is_budget(c) ? "frame_format" : seq_is_jpeg(c) ? "jpeg_count" : seq_is_png(c) ? "png_seq_count" : "pal8_seq_hist"; }
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
    if (c->timing == 1) tm.mark(seq_pass_mark(c));
    return POPPY_OK;
}

int seq_abort(poppy_hip_ctx* c) {
    c->seq.open = false;
    int rc = drain_frames(c);
    if (c->seq.tables && hipMemset(c->seq.tables, 0, kPal8SeqTableOffset) != hipSuccess && rc == POPPY_OK) rc = fail(c, POPPY_E_DEVICE, "could not clear the sequence tables");
    if (c->seq.jpeg && hipMemset(c->seq.jpeg, 0, sizeof(jpeg::SymbolCounts)) != hipSuccess && rc == POPPY_OK) rc = fail(c, POPPY_E_DEVICE, "could not clear the sequence's symbol counts");
    if (c->seq.png && hipMemset(c->seq.png, 0, kPngSeqSumWords * 4) != hipSuccess && rc == POPPY_OK) rc = fail(c, POPPY_E_DEVICE, "could not clear the sequence's token counts");
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
// ... and of one frame of a JPEG sequence: from its planes (its place in a sequence store) on the sequence's built tables, the OPT forms of the coder and the gather
static void enqueue_seq_jpeg_coding(const uint8_t* planes, const void* tables, const void* built, uint8_t* scratch, uint8_t* frame, void* total_dev, int W, int H, jpeg::Sampling sm, hipStream_t s, Timer* tm) {
    launch_jpeg_code_on(planes, tables, built, scratch, W, H, sm, s);
    if (tm) tm->mark("jpeg_code");
    launch_jpeg_pack_on(tables, built, scratch, frame, (uint32_t*)total_dev, W, H, sm, s);
    if (tm) tm->mark("jpeg_pack");
}

// ... and of one frame of a PNG sequence: the choice among nine, then PNG_RUNS' scan, the pack on the sequence's table, the CRC and the finish, all on the frame's place
// in the store, which is its coder's scratch and holds its filtered stream
static void enqueue_seq_png_coding(uint8_t* place, const void* table, uint8_t* frame, void* total_dev, int W, int H, hipStream_t s, Timer* tm) {
    launch_png_seq_cost(place, table, W, H, s);
    if (tm) tm->mark("png_seq_cost");
    launch_png_scan(place, frame, W, H, png::kRunsSeq, s);
    if (tm) tm->mark("png_scan");
    launch_png_seq_pack(place, table, frame, W, H, s);
    if (tm) tm->mark("png_seq_pack");
    launch_png_crc(place, frame, W, H, png::kRunsSeq, s);
    if (tm) tm->mark("png_crc");
    launch_png_finish(place, frame, (uint32_t*)total_dev, W, H, png::kRunsSeq, s);
    if (tm) tm->mark("png_finish");
}

// ... and of one frame of a sequence under a sequence budget: from its planes on the tables of all qualities, the picked quality read from the sequence's search state
static void enqueue_seq_jpeg_budget_coding(const uint8_t* planes, const JpegBudget& budget, const uint8_t* state, uint8_t* scratch, uint8_t* frame, void* total_dev, int W, int H, jpeg::Sampling sm, hipStream_t s, Timer* tm) {
    launch_jpeg_code_picked_by(planes, budget, state, scratch, W, H, sm, s);
    if (tm) tm->mark("jpeg_code");
    launch_jpeg_pack_picked_by(budget, state, scratch, frame, (uint32_t*)total_dev, W, H, sm, s);
    if (tm) tm->mark("jpeg_pack");
}
// the sequence budget's search over a store of n frames of planes: kJpegBudgetSteps steps of one measuring launch over segments x frames and one pick, a fixed
// sequence of dispatches whatever the search finds; behind it `state` holds the one quality
static void enqueue_seq_jpeg_budget_search(const uint8_t* store, size_t stride, int n, const JpegBudget& budget, uint8_t* state, int W, int H, jpeg::Sampling sm, hipStream_t s, Timer* tm) {
    for (int step = 0; step < kJpegBudgetSteps; ++step) {
        launch_jpeg_seq_measure(store, stride, n, budget, state, step, W, H, sm, s);
        if (tm) tm->mark("jpeg_measure");
        launch_jpeg_seq_pick(budget, state, n, step, W, H, sm, s);
        if (tm) tm->mark("jpeg_pick");
    }
}

// Every frame of a coded sequence: coded from its place in the store (GIF_SEQ: k_gif_lzw_bgr, no index plane; the JPEG sequences: k_jpeg_code and k_jpeg_pack in their
// OPT forms on the sequence's tables) into one of R device buffers, each followed by the coder's scratch, on the ring buffer's own stream; the coder's last kernel
// stores the frame's length into the ring buffer's pinned word.  The host waits for that stream, reads the word, bounds-checks it
// as slot_frame_length does and queues the copy of exactly that many bytes on the same stream — no event behind a copy.  Frame k + 1 is being coded (on the next ring
// buffer's stream) while the host waits for frame k's length, its copy runs and the writer has the frames before it; the writer gets the frames in order.
static int seq_hand_over_coded(poppy_hip_ctx* c, poppy_write_cb write, void* user) {
    PaletteSeq& q = c->seq;
    const WriterGeom g = writer_geom(c);
    const int n = q.count, W = g.w, H = g.h;
    const bool marks = c->timing == 1;
    const FormatTraits& t = writer_traits(c, c->frame_format);
    JpegBudget seq_budget;
    if (seq_is_budget(c)) { int rc = context_jpeg_seq_budget(c, &seq_budget); if (rc) return rc; }
    const size_t capacity = poppy_frame_bytes(t.format, W, H), frame_part = (capacity + 16 + 255) & ~(size_t)255;
    const size_t each = frame_part + (t.coder == kCoderPng ? 0 : (coding_scratch_bytes(t, W, H) + 255) & ~(size_t)255);      // (a PNG frame's scratch is its place in the store)
    WriterRing ring;
    { int rc = ring.open(c, capacity, false); if (rc) return rc; }
    HIPCHK(c, q.coded.reserve(each * ring.R));
    if (!q.coded_total) {
        HIPCHK(c, hipHostMalloc((void**)&q.coded_total, 64 * poppy_hip_ctx::kStageRing, hipHostMallocMapped));
        HIPCHK(c, hipHostGetDevicePointer((void**)&q.coded_total_dev, q.coded_total, 0));
    }
    auto d_frame = [&](int k) { return q.coded.p + (size_t)(k % ring.R) * each; };
    auto total_word = [&](int k) { return (volatile uint32_t*)((uint8_t*)q.coded_total + 64 * (size_t)(k % ring.R)); };
#ifdef POPPY_EXPERIMENTS
    const size_t plane = ((size_t)W * H + 255) & ~(size_t)255;
    HIPCHK(c, q.idx.reserve(plane * ring.R));
    const bool two_dispatch = t.coder == kCoderGif && getenv("POPPY_GIF_SEQ_TWO_DISPATCH") != nullptr;      // timing experiment, read per sequence so that one process alternates: the index plane through HBM (k_pal8_remap, then k_gif_lzw); the same bytes
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
            launch_gif_pack_seq(q.tables, d_frame(k) + frame_part, d_frame(k), (uint32_t*)(q.coded_total_dev + 64 * (size_t)(k % ring.R)), W, H, s);
            if (marks) tm.mark("gif_pack");
        } else
#endif
        if (t.coder == kCoderPng) enqueue_seq_png_coding(q.store.p + (size_t)k * q.stride, seq_png_table(q), d_frame(k), q.coded_total_dev + 64 * (size_t)(k % ring.R), W, H, s, marks ? &tm : nullptr);
        else if (seq_budget) enqueue_seq_jpeg_budget_coding(q.store.p + (size_t)k * q.stride, seq_budget, q.budget.p, d_frame(k) + frame_part, d_frame(k), q.coded_total_dev + 64 * (size_t)(k % ring.R), W, H, t.sampling(), s, marks ? &tm : nullptr);
        else if (t.coder == kCoderJpeg) enqueue_seq_jpeg_coding(q.store.p + (size_t)k * q.stride, c->jpeg_tables, seq_jpeg_built(q), d_frame(k) + frame_part, d_frame(k), q.coded_total_dev + 64 * (size_t)(k % ring.R), W, H, t.sampling(), s, marks ? &tm : nullptr);
        else enqueue_seq_gif_coding(q.store.p + (size_t)k * q.stride, q.tables, d_frame(k) + frame_part, d_frame(k), q.coded_total_dev + 64 * (size_t)(k % ring.R), W, H, s, marks ? &tm : nullptr);
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
        if (!coded_length_ok(total, capacity, t.least)) return fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds");
        HIPCHK(c, hipMemcpyAsync(ring.buffer(k), d_frame(k), total, hipMemcpyDeviceToHost, s));
        ++ring.issued;
        return POPPY_OK;
    };
    auto deliver = [&]() -> int {
        if (ring.issued == ring.written) { int rc = copy_next(); if (rc) return rc; }
        uint8_t* frame = nullptr;
        HIPCHK(c, ring.deliver_next(c, false, &frame));
        write(user, frame, W, H, writer_stride(t.format, W));
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
    if (seq_is_budget(c)) {                                        // the one search over the store, in place of a build
        const WriterGeom g = writer_geom(c);
        JpegBudget budget;
        { int rc = context_jpeg_seq_budget(c, &budget); if (rc) return rc; }
        Timer tm(c, c->stream);
        if (c->timing == 1) tm.mark(nullptr);
        enqueue_seq_jpeg_budget_search(q.store.p, q.stride, q.count, budget, q.budget.p, g.w, g.h, writer_traits(c, c->frame_format).sampling(), c->stream, c->timing == 1 ? &tm : nullptr);
    } else {
        Timer tm(c, c->stream);
        if (c->timing == 1) tm.mark(nullptr);
        if (seq_is_png(c)) launch_png_seq_table(seq_png_sums(q), seq_png_table(q), c->stream);      // once, on the sums: they are zero behind it
        else if (seq_is_jpeg(c)) launch_jpeg_table_build(seq_jpeg_counts(q), const_cast<void*>(seq_jpeg_built(q)), c->stream);      // once, on the sums: the counts are zero behind it
        else launch_pal8_seq_build(q.tables, c->stream);
        if (c->timing == 1) tm.mark(seq_is_png(c) ? "png_seq_table" : seq_is_jpeg(c) ? "jpeg_tables" : "pal8_seq_build");
    }
    HIPCHK(c, hipGetLastError());
    if (!writer_traits(c, c->frame_format).coded()) return seq_hand_over_indices(c, write, user);
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

// the body of poppy_hip_bgr_frames_to_jpeg_seq_frames and its 4:4:4 twin: host BGR frames up one by one, each through the pass of a JPEG sequence (raster kernel,
// counting kernel) into a store of planes, one table build, every frame coded and `total` bytes of it down — all on buffers and tables that live for the call
static int jpeg_seq_code_host_frames(poppy_hip_ctx* c, int fmt, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int W, int H, int quality, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    if (!bgr || !dst || W <= 0 || H <= 0 || stride < (size_t)W * 3 || n_frames < 1 || quality < 1 || quality > 100) return fail(c, POPPY_E_ARG, "bad arguments");
    if (frame_stride < stride * ((size_t)H - 1) + (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad arguments: the frames overlap");
    if (const char* why = sequence_refuses(fmt, n_frames, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    HIPCHK(c, hipSetDevice(c->device));
    // everything lives for the call: the context's own sequence tables, store and rings, and its quality's tables, are not touched
    const FormatTraits& t = *format_traits(fmt);
    const jpeg::Sampling sm = t.sampling();
    const size_t row = (size_t)W * 3, place = (raster_bytes(t.raster, (size_t)W, (size_t)H) + 15) & ~(size_t)15, capacity = poppy_frame_bytes(fmt, W, H);
    jpeg::QualityTables qt;
    jpeg::fill_quality_tables(quality, &qt);
    CallBuffers held;
    uint8_t *d_bgr = nullptr, *store = nullptr, *seq = nullptr, *d_tables = nullptr, *work = nullptr, *frame = nullptr;
    hipError_t e = held.alloc(&d_bgr, row * H + 16);
    if (e == hipSuccess) e = held.alloc(&store, place * (size_t)n_frames);
    if (e == hipSuccess) e = held.alloc(&seq, kJpegSeqTableBytes);
    if (e == hipSuccess) e = held.alloc(&d_tables, kJpegTableBytes);
    if (e == hipSuccess) e = held.alloc(&work, jpeg_scratch_bytes(W, H, sm, true));
    if (e == hipSuccess) e = held.alloc(&frame, capacity + 16);
    if (e == hipSuccess) e = hipMemsetAsync(seq, 0, kJpegSeqTableBytes, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tables, &qt, sizeof qt, hipMemcpyHostToDevice, c->stream);
    for (int k = 0; k < n_frames && e == hipSuccess; ++k) {      // (the one BGR buffer: the upload is ordered behind the raster kernel that read the frame before)
        e = copy_rows_async(d_bgr, row, bgr + (size_t)k * frame_stride, stride, row, (size_t)H, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) break;
        (sm == jpeg::k444 ? launch_bgr_to_i444 : launch_bgr_to_i420)(d_bgr, store + (size_t)k * place, W, H, c->stream, nullptr);
        launch_jpeg_count_into(store + (size_t)k * place, d_tables, (uint32_t*)seq, W, H, sm, c->stream);
        e = hipGetLastError();
    }
    const void* built = seq + sizeof(jpeg::SymbolCounts);
    if (e == hipSuccess) { launch_jpeg_table_build((uint32_t*)seq, const_cast<void*>(built), c->stream); e = hipGetLastError(); }
    int rc = POPPY_OK;
    for (int k = 0; k < n_frames && e == hipSuccess && rc == POPPY_OK; ++k) {
        uint32_t total = 0;
        enqueue_seq_jpeg_coding(store + (size_t)k * place, d_tables, built, work, frame, nullptr, W, H, sm, c->stream, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&total, frame, 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess && !coded_length_ok(total, capacity, t.least)) rc = fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds");
        else if (e == hipSuccess) e = hipMemcpy(dst + (size_t)k * capacity, frame, total, hipMemcpyDeviceToHost);
    }
    (void)hipStreamSynchronize(c->stream);                         // nothing of the call is in flight when its buffers and `qt` go (`held`, at the return)
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("JPEG sequence coding: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return rc;
}
int poppy_hip_bgr_frames_to_jpeg_seq_frames(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int W, int H, int quality, uint8_t* dst) {
    return jpeg_seq_code_host_frames(c, POPPY_FRAME_JPEG_SEQ, bgr, stride, frame_stride, n_frames, W, H, quality, dst);
}
int poppy_hip_bgr_frames_to_jpeg444_seq_frames(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int W, int H, int quality, uint8_t* dst) {
    return jpeg_seq_code_host_frames(c, POPPY_FRAME_JPEG444_SEQ, bgr, stride, frame_stride, n_frames, W, H, quality, dst);
}

// the body of poppy_hip_bgr_frames_to_jpeg_seq_budget_frames and its 4:4:4 twin: host BGR frames up one by one, each through the raster kernel into a store of
// planes, the sequence budget's search once over the store on the call's own words, every frame coded at the picked quality and `total` bytes of it down — all on
// buffers that live for the call; of the context only its tables of all qualities are used, and its own budgets and quality are neither read nor touched
static int jpeg_seq_budget_code_host_frames(poppy_hip_ctx* c, int fmt, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int W, int H, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used) {
    if (!c) return POPPY_E_ARG;
    if (!bgr || !dst || W <= 0 || H <= 0 || stride < (size_t)W * 3 || n_frames < 1 || quality_max < 1 || quality_max > 100 || budget == 0) return fail(c, POPPY_E_ARG, "bad arguments");
    if (frame_stride < stride * ((size_t)H - 1) + (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad arguments: the frames overlap");
    if (const char* why = format_refuses(fmt, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = ensure_jpeg_budget_tables(c); if (rc) return rc; }
    const FormatTraits& t = *format_traits(fmt);
    const jpeg::Sampling sm = t.sampling();
    const size_t row = (size_t)W * 3, place = (raster_bytes(t.raster, (size_t)W, (size_t)H) + 15) & ~(size_t)15, capacity = poppy_frame_bytes(fmt, W, H);
    const JpegSeqBudgetParams p{(uint32_t)budget, (uint32_t)quality_max, (uint32_t)(budget >> 32), 0};
    CallBuffers held;
    uint8_t *d_bgr = nullptr, *store = nullptr, *state = nullptr, *d_params = nullptr, *work = nullptr, *frame = nullptr;
    hipError_t e = held.alloc(&d_bgr, row * H + 16);
    if (e == hipSuccess) e = held.alloc(&store, place * (size_t)n_frames);
    if (e == hipSuccess) e = held.alloc(&state, jpeg_seq_budget_bytes(n_frames, W, H, sm));
    if (e == hipSuccess) e = held.alloc(&d_params, sizeof p);
    if (e == hipSuccess) e = held.alloc(&work, jpeg_scratch_bytes(W, H, sm, false));
    if (e == hipSuccess) e = held.alloc(&frame, capacity + 16);
    if (e == hipSuccess) e = hipMemcpyAsync(d_params, &p, sizeof p, hipMemcpyHostToDevice, c->stream);
    JpegBudget of_call;
    of_call.tables = c->jpeg_budget_tables; of_call.params = d_params;
    for (int k = 0; k < n_frames && e == hipSuccess; ++k) {      // (the one BGR buffer: the upload is ordered behind the raster kernel that read the frame before)
        e = copy_rows_async(d_bgr, row, bgr + (size_t)k * frame_stride, stride, row, (size_t)H, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) break;
        (sm == jpeg::k444 ? launch_bgr_to_i444 : launch_bgr_to_i420)(d_bgr, store + (size_t)k * place, W, H, c->stream, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) { enqueue_seq_jpeg_budget_search(store, place, n_frames, of_call, state, W, H, sm, c->stream, nullptr); e = hipGetLastError(); }
    int rc = POPPY_OK;
    for (int k = 0; k < n_frames && e == hipSuccess && rc == POPPY_OK; ++k) {
        uint32_t total = 0;
        enqueue_seq_jpeg_budget_coding(store + (size_t)k * place, of_call, state, work, frame, nullptr, W, H, sm, c->stream, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&total, frame, 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess && !coded_length_ok(total, capacity, t.least)) rc = fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds");
        else if (e == hipSuccess) e = hipMemcpy(dst + (size_t)k * capacity, frame, total, hipMemcpyDeviceToHost);
    }
    (void)hipStreamSynchronize(c->stream);                         // nothing of the call is in flight when its buffers and `p` go (`held`, at the return)
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("JPEG sequence budget coding: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    if (rc == POPPY_OK && quality_used) *quality_used = poppy_jpeg_frame_quality(dst);
    return rc;
}
int poppy_hip_bgr_frames_to_jpeg_seq_budget_frames(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int W, int H, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used) {
    return jpeg_seq_budget_code_host_frames(c, POPPY_FRAME_JPEG, bgr, stride, frame_stride, n_frames, W, H, quality_max, budget, dst, quality_used);
}
int poppy_hip_bgr_frames_to_jpeg444_seq_budget_frames(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int W, int H, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used) {
    return jpeg_seq_budget_code_host_frames(c, POPPY_FRAME_JPEG444, bgr, stride, frame_stride, n_frames, W, H, quality_max, budget, dst, quality_used);
}

// host BGR frames up one by one, each through the pass of a PNG sequence (filter, counting kernel) into a store of places, one table build, every frame coded on its
// place and `total` bytes of it down — all on buffers and sums that live for the call: the context's own sequence, store and rings are not touched
int poppy_hip_bgr_frames_to_png_seq_frames(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int W, int H, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    if (!bgr || !dst || W <= 0 || H <= 0 || stride < (size_t)W * 3 || n_frames < 1) return fail(c, POPPY_E_ARG, "bad arguments");
    if (frame_stride < stride * ((size_t)H - 1) + (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad arguments: the frames overlap");
    if (const char* why = sequence_refuses(POPPY_FRAME_PNG_SEQ, n_frames, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    HIPCHK(c, hipSetDevice(c->device));
    const FormatTraits& t = *format_traits(POPPY_FRAME_PNG_SEQ);
    const size_t row = (size_t)W * 3, place = (png_scratch_bytes(W, H, t.variant) + 15) & ~(size_t)15, capacity = poppy_frame_bytes(POPPY_FRAME_PNG_SEQ, W, H);
    CallBuffers held;
    uint8_t *d_bgr = nullptr, *store = nullptr, *seq = nullptr, *frame = nullptr;
    hipError_t e = held.alloc(&d_bgr, row * H + 16);
    if (e == hipSuccess) e = held.alloc(&store, place * (size_t)n_frames);
    if (e == hipSuccess) e = held.alloc(&seq, kPngSeqTableBytes);
    if (e == hipSuccess) e = held.alloc(&frame, capacity + 16);
    if (e == hipSuccess) e = hipMemsetAsync(seq, 0, kPngSeqTableBytes, c->stream);
    for (int k = 0; k < n_frames && e == hipSuccess; ++k) {      // (the one BGR buffer: the upload is ordered behind the filter that read the frame before)
        e = copy_rows_async(d_bgr, row, bgr + (size_t)k * frame_stride, stride, row, (size_t)H, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) break;
        launch_png_filter(d_bgr, store + (size_t)k * place, W, H, t.variant, c->stream);
        launch_png_seq_count(store + (size_t)k * place, (uint32_t*)seq, W, H, c->stream);
        e = hipGetLastError();
    }
    void* table = seq + kPngSeqSumWords * 4;
    if (e == hipSuccess) { launch_png_seq_table((uint32_t*)seq, table, c->stream); e = hipGetLastError(); }
    int rc = POPPY_OK;
    for (int k = 0; k < n_frames && e == hipSuccess && rc == POPPY_OK; ++k) {
        uint32_t total = 0;
        enqueue_seq_png_coding(store + (size_t)k * place, table, frame, nullptr, W, H, c->stream, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&total, frame, 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess && !coded_length_ok(total, capacity, t.least)) rc = fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds");
        else if (e == hipSuccess) e = hipMemcpy(dst + (size_t)k * capacity, frame, total, hipMemcpyDeviceToHost);
    }
    (void)hipStreamSynchronize(c->stream);                         // nothing of the call is in flight when its buffers go (`held`, at the return)
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("PNG sequence coding: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return rc;
}

// k_png_seq_table alone on given counts: what poppy_png_seq_table gives, with its refusals
int poppy_hip_png_seq_table(poppy_hip_ctx* c, const uint32_t* counts, uint8_t* lengths, uint8_t* header_bits, int* n_header_bits) {
    if (!c) return POPPY_E_ARG;
    if (poppy_png_seq_table(counts, nullptr, nullptr, nullptr) != POPPY_OK)      // (the refusals are the host statement's; its outputs are not used)
        return fail(c, POPPY_E_ARG, "bad arguments: a null pointer, counts that are all zero, whose sum is 2^32 or more, or no count for symbol 256");
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t padded[kPngSeqSumWords] = {};
    memcpy(padded, counts, sizeof(uint32_t) * png_opt::kSymbols);
    png_opt::OwnTable built;
    CallBuffers held;
    uint8_t* seq = nullptr;
    HIPCHK(c, held.alloc(&seq, kPngSeqTableBytes));
    uint8_t* table = seq + kPngSeqSumWords * 4;
    hipError_t e = hipMemcpyAsync(seq, padded, sizeof padded, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch_png_seq_table((uint32_t*)seq, table, c->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(&built, table, sizeof built, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);     // nothing of the call is in flight when its buffers go (`held`, at the return)
    if (e == hipSuccess) e = e_sync;
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("PNG sequence table build: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    if (built.header_bits < 17 || built.header_bits > (uint32_t)png_opt::kOwnHeaderBitsMax) return fail(c, POPPY_E_DEVICE, "the built header's length is outside its bounds");
    if (lengths) for (int i = 0; i < png_opt::kSymbols; ++i) lengths[i] = (uint8_t)(built.code[i] & 15u);
    if (header_bits) {
        memset(header_bits, 0, POPPY_PNG_SEQ_HEADER_BYTES);
        for (uint32_t i = 0; 8 * i < built.header_bits; ++i) header_bits[i] = (uint8_t)(built.header[i / 4] >> (8 * (i & 3)));
    }
    if (n_header_bits) *n_header_bits = (int)built.header_bits;
    return POPPY_OK;
}

}  // extern "C"
