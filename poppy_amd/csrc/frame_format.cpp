// frame_format.cpp — everything that depends on the format a writer gets its frames in (frame_format.h).  The frame path itself — which stream a frame's
// conversion runs on, what its completion event rides on, when its copy is issued — is frame_render.cpp's and frame_sequence.cpp's (enqueue_body, render_slot, render_sequence_frames).
#include "context.h"

static bool pal8_fits(int W, int H) { return (unsigned long long)W * (unsigned long long)H <= (unsigned long long)POPPY_PAL8_MAX_PIXELS; }
constexpr const char* kPal8SizeMsg = "POPPY_FRAME_PAL8, POPPY_FRAME_PAL8_SEQ, POPPY_FRAME_GIF and POPPY_FRAME_GIF_SEQ take frames of at most 2^24 pixels";
constexpr const char* kGifSizeMsg = "POPPY_FRAME_GIF and POPPY_FRAME_GIF_SEQ take frames of at most 65535 pixels in width and height";
constexpr const char* kSeqSizeMsg = "POPPY_FRAME_PAL8_SEQ and POPPY_FRAME_GIF_SEQ take sequences of fewer than 2^32 pixels in all";

bool format_known(int fmt) {
    return fmt == POPPY_FRAME_BGR || fmt == POPPY_FRAME_I420 || fmt == POPPY_FRAME_PAL8 || fmt == POPPY_FRAME_PAL8_SEQ || fmt == POPPY_FRAME_GIF || fmt == POPPY_FRAME_GIF_SEQ;
}
const char* format_refuses(int fmt, int W, int H) {
    if ((format_builds_palette(fmt) || format_is_sequence(fmt)) && !pal8_fits(W, H)) return kPal8SizeMsg;
    if (format_is_coded(fmt) && (W > 65535 || H > 65535)) return kGifSizeMsg;
    return nullptr;
}
static const char* sequence_refuses(int fmt, int n, int W, int H) {
    if (const char* why = format_refuses(fmt, W, H)) return why;
    return (unsigned long long)n * (unsigned long long)W * (unsigned long long)H >= POPPY_PAL8_SEQ_MAX_PIXELS ? kSeqSizeMsg : nullptr;
}
size_t writer_stride(int fmt, int W) { return format_is_coded(fmt) ? 0 : fmt == POPPY_FRAME_BGR ? (size_t)W * 3 : (size_t)W; }
constexpr const char* kSizeMsg = "the frame size set with poppy_hip_set_frame_size takes frames at least as large and at most 8 times as large per side";
WriterGeom scaled_geom(int W, int H, int scale) { return WriterGeom{(W + scale - 1) / scale, (H + scale - 1) / scale, scale, scale > 1 ? kScaleFactor : kScaleNone}; }
WriterGeom sized_geom(int ow, int oh) { return WriterGeom{ow, oh, 1, kScaleSize}; }
bool size_admits(int W, int H, int ow, int oh) {
    return ow >= 1 && oh >= 1 && ow <= W && oh <= H && (long long)W <= (long long)POPPY_FRAME_SCALE_MAX * ow && (long long)H <= (long long)POPPY_FRAME_SCALE_MAX * oh;
}
WriterGeom context_geom(const poppy_hip_ctx* c, int W, int H, bool has_writer) {
    return has_writer && c->frame_ow ? sized_geom(c->frame_ow, c->frame_oh) : scaled_geom(W, H, has_writer ? c->frame_scale : 1);
}
WriterGeom writer_geom(const poppy_hip_ctx* c, bool has_writer) { return context_geom(c, c->W, c->H, has_writer); }
const char* writer_refuses(const poppy_hip_ctx* c, int fmt, int W, int H) {
    if (c->frame_ow && !size_admits(W, H, c->frame_ow, c->frame_oh)) return kSizeMsg;
    const WriterGeom g = context_geom(c, W, H);
    return format_refuses(fmt, g.w, g.h);
}
void launch_writer_scaling(const WriterGeom& g, const uint8_t* src, uint8_t* dst, int W, int H, hipStream_t s, hipEvent_t done) {
    if (g.kind == kScaleSize) launch_bgr_resize_area(src, dst, W, H, g.w, g.h, s, done);
    else launch_bgr_downscale(src, dst, W, H, g.scale, s, done);
}
const char* scaling_mark(const WriterGeom& g) { return g.kind == kScaleSize ? "frame_resize" : "frame_scale"; }
int writer_format(const poppy_hip_ctx* c, bool has_writer) { return has_writer ? c->frame_format : POPPY_FRAME_BGR; }
bool writer_wants_sequence(const poppy_hip_ctx* c, bool has_writer) { return has_writer && format_is_sequence(c->frame_format); }

// conversion tables, zero before the first frame (the palette builds leave them zero again): PAL8's per slot and for the scratch, the sequence's per context
static int alloc_zeroed_tables(poppy_hip_ctx* c, uint8_t** tables, size_t bytes) {
    if (*tables) return POPPY_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (!prepare_pal8()) return fail(c, POPPY_E_DEVICE, "could not raise the palette build's LDS limit");      // (per device: kernels.h)
    HIPCHK(c, hipMalloc((void**)tables, bytes));
    HIPCHK(c, hipMemset(*tables, 0, bytes));
    return POPPY_OK;
}

// a slot's conversion side stream and the event that rides on its unsharp (the palette formats; they live as long as the context)
static int alloc_slot_side(poppy_hip_ctx* c, SlotFormat& f) {
    // The side streams are created at the LOWEST stream priority.  The runtime keeps its hardware queues per priority, so they never share a queue with the
    // chain's stream or the plan upload's (normal priority): a dispatch waits for the one before it in its hardware queue whatever its stream, and a
    // 350 us palette build in the chain's queue held the next frame's warp back for its whole length (kernel trace).
    if (!f.fmt_stream) {
        int least = 0, greatest = 0;
        HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(c, hipStreamCreateWithPriority(&f.fmt_stream, hipStreamNonBlocking, least));
    }
    if (!f.bgr_done) HIPCHK(c, hipEventCreateWithFlags(&f.bgr_done, hipEventDisableTiming));
    return POPPY_OK;
}

// I420: the slot's I420 buffer.  PAL8: its PAL8 buffer, tables, side stream and event.  GIF: PAL8's (the coder reads the slot's PAL8 frame) and the coded frame, the
// coder's scratch and the pinned length word.  PAL8_SEQ and GIF_SEQ: the slots' side streams and the context's sequence tables — the store and the index ring depend on the
// sequence's length and, under GIF_SEQ, the ring of coded frames: seq_begin, seq_finish.  All of it in the writer's geometry; with a scale above 1 or a size the scaled BGR frame too.
int alloc_slot_format(poppy_hip_ctx* c) {
    const WriterGeom g = writer_geom(c);
    const int fmt = c->frame_format, W = g.w, H = g.h;
    if (const char* why = writer_refuses(c, fmt, c->W, c->H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    for (FrameSlot& slot : c->slots) {
        SlotFormat& f = slot.fmt;
        if (g.scaled() && !f.scaled) HIPCHK(c, hipMalloc((void**)&f.scaled, poppy_frame_bytes(POPPY_FRAME_BGR, W, H) + 16));
        if (fmt == POPPY_FRAME_I420 && !f.i420) HIPCHK(c, hipMalloc((void**)&f.i420, poppy_frame_bytes(fmt, W, H) + 16));
        if (format_builds_palette(fmt)) {
            if (!f.pal8) HIPCHK(c, hipMalloc((void**)&f.pal8, poppy_frame_bytes(POPPY_FRAME_PAL8, W, H) + 16));
            int rc = alloc_zeroed_tables(c, &f.pal8_tables, kPal8TableBytes); if (rc) return rc;
        }
        if (format_builds_palette(fmt) || format_is_sequence(fmt)) { int rc = alloc_slot_side(c, f); if (rc) return rc; }
        if (fmt != POPPY_FRAME_GIF) continue;                       // (the slot's coded frame: GIF_SEQ codes from the store into the sequence's ring)
        if (!f.gif) HIPCHK(c, hipMalloc((void**)&f.gif, poppy_frame_bytes(fmt, W, H) + 16));
        if (!f.gif_scratch) HIPCHK(c, hipMalloc((void**)&f.gif_scratch, gif_scratch_bytes(W, H)));
        if (!f.gif_total) {
            HIPCHK(c, hipHostMalloc((void**)&f.gif_total, 64, hipHostMallocMapped));
            HIPCHK(c, hipHostGetDevicePointer(&f.gif_total_dev, f.gif_total, 0));
            *f.gif_total = 0;
        }
    }
    return format_is_sequence(fmt) ? alloc_zeroed_tables(c, &c->seq.tables, kPal8SeqTableBytes) : POPPY_OK;
}

void free_slot_format_pair(SlotFormat& f) {
    for (uint8_t* b : {f.scaled, f.i420, f.pal8, f.pal8_tables, f.gif, f.gif_scratch}) if (b) (void)hipFree(b);
    f.scaled = f.i420 = f.pal8 = f.pal8_tables = f.gif = f.gif_scratch = nullptr;
    if (f.gif_total) (void)hipHostFree(f.gif_total);
    f.gif_total = nullptr; f.gif_total_dev = nullptr;
}
void free_slot_format_ctx(SlotFormat& f) {
    if (f.fmt_stream) (void)hipStreamDestroy(f.fmt_stream);
    if (f.bgr_done) (void)hipEventDestroy(f.bgr_done);
}
void free_context_format(poppy_hip_ctx* c) {
    for (uint8_t* b : {c->scale_scratch, c->fmt_scratch, c->fmt_scratch_tables, c->seq.tables, c->seq.store, c->seq.idx, c->seq.gif}) if (b) (void)hipFree(b);
    if (c->seq.gif_total) (void)hipHostFree(c->seq.gif_total);
    c->scale_scratch = c->fmt_scratch = c->fmt_scratch_tables = nullptr; c->scale_scratch_bytes = c->fmt_scratch_bytes = 0;
    c->seq = PaletteSeq();
}

bool slot_format_ready(const poppy_hip_ctx* c, const FrameSlot& slot, int fmt, const WriterGeom& g) {
    const SlotFormat& f = slot.fmt;
    if (g.scaled() && !f.scaled) return false;
    if (fmt == POPPY_FRAME_I420) return f.i420 != nullptr;
    if (format_is_sequence(fmt)) return c->seq.open && c->seq.tables && f.fmt_stream && f.bgr_done;
    if (format_builds_palette(fmt) && !(f.pal8 && f.pal8_tables && f.fmt_stream && f.bgr_done)) return false;
    return fmt != POPPY_FRAME_GIF || (f.gif && f.gif_scratch && f.gif_total);
}
const uint8_t* slot_bgr(const FrameSlot& f, const WriterGeom& g) { return g.scaled() ? f.fmt.scaled : f.out; }
const uint8_t* slot_frame(const FrameSlot& f, int fmt, const WriterGeom& g) {
    return fmt == POPPY_FRAME_I420 ? f.fmt.i420 : fmt == POPPY_FRAME_PAL8 ? f.fmt.pal8 : fmt == POPPY_FRAME_GIF ? f.fmt.gif : slot_bgr(f, g);
}
bool slot_frame_length(const FrameSlot& f, int fmt, size_t capacity, size_t* bytes) {
    *bytes = format_is_coded(fmt) ? *(volatile uint32_t*)f.fmt.gif_total : capacity;
    return *bytes <= capacity && (!format_is_coded(fmt) || *bytes >= 776);
}

// the GIF half: the PAL8 frame coded into `frame`, its length also into the pinned word behind total_dev (null: none); `done` rides on the second dispatch
static void enqueue_gif_coding(const uint8_t* pal8, uint8_t* scratch, uint8_t* frame, void* total_dev, int W, int H, hipStream_t s, hipEvent_t done, Timer* tm) {
    launch_gif_lzw(pal8, scratch, W, H, s);
    if (tm) tm->mark("gif_lzw");
    launch_gif_pack(pal8, scratch, frame, (uint32_t*)total_dev, W, H, s, done);
    if (tm) tm->mark("gif_pack");
}

void enqueue_conversion(int fmt, const WriterGeom& g, const uint8_t* src_bgr, int W, int H, const SlotFormat& b, hipStream_t s, hipEvent_t done, Timer* tm) {
    if (g.scaled()) {                                              // the conversion's first dispatch; what follows reads the scaled frame
        launch_writer_scaling(g, src_bgr, b.scaled, W, H, s, fmt == POPPY_FRAME_BGR ? done : nullptr);
        if (tm) tm->mark(scaling_mark(g));
        src_bgr = b.scaled; W = g.w; H = g.h;
    }
    if (fmt == POPPY_FRAME_I420) {
        launch_bgr_to_i420(src_bgr, b.i420, W, H, s, done);
        if (tm) tm->mark("frame_format");
    } else if (format_builds_palette(fmt)) {
        // PAL8 is three dispatches, and the palette build in the middle is one workgroup's serial work (about as long as the rest of the frame)
        const bool gif = fmt == POPPY_FRAME_GIF;
        launch_pal8_hist(src_bgr, b.pal8_tables, W, H, s);
        if (tm) tm->mark("pal8_hist");
        launch_pal8_build(b.pal8_tables, b.pal8, W, H, s);
        if (tm) tm->mark("pal8_build");
        launch_pal8_remap(src_bgr, b.pal8_tables, b.pal8, W, H, s, gif ? nullptr : done);
        if (tm) tm->mark("frame_format");                      // (under PAL8 and GIF: the index plane alone)
        if (gif) enqueue_gif_coding(b.pal8, b.gif_scratch, b.gif, b.gif_total_dev, W, H, s, done, tm);
    }
}

int seq_begin(poppy_hip_ctx* c, int n) {
    const WriterGeom g = writer_geom(c);
    const int W = g.w, H = g.h;
    PaletteSeq& q = c->seq;
    if (q.open) { int rc = seq_abort(c); if (rc) return rc; }      // (a sequence that a device error left open: its frames and sums are dropped, not mixed into this one)
    if (const char* why = sequence_refuses(c->frame_format, n, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);      // (a sequence format: writer_wants_sequence)
    { int rc = alloc_slot_format(c); if (rc) return rc; }
    const size_t stride = ((size_t)W * H * 3 + 15) & ~(size_t)15, need = stride * (size_t)n;      // (every frame's place begins on a 16-byte boundary)
    if (need > q.store_bytes) {
        if (q.store) (void)hipFree(q.store);
        q.store = nullptr; q.store_bytes = 0;
        if (hipMalloc((void**)&q.store, need) != hipSuccess) { (void)hipGetLastError(); return fail(c, POPPY_E_DEVICE, "no device memory for the sequence's frames (3 * width * height bytes each)"); }
        q.store_bytes = need;
    }
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
uint8_t* seq_next_place(poppy_hip_ctx* c) { return c->seq.count < c->seq.n ? c->seq.store + (size_t)c->seq.count++ * c->seq.stride : nullptr; }

// a full-size device frame scaled down into the context's scale scratch on c->stream (grown when needed: the stream's order keeps the readers of one frame
// in front of the next frame's downscale)
static int scale_into_scratch(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, const WriterGeom& g) {
    const size_t bytes = poppy_frame_bytes(POPPY_FRAME_BGR, g.w, g.h) + 16;
    if (bytes > c->scale_scratch_bytes) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->scale_scratch) (void)hipFree(c->scale_scratch);
        c->scale_scratch = nullptr; c->scale_scratch_bytes = 0;
        HIPCHK(c, hipMalloc((void**)&c->scale_scratch, bytes));
        c->scale_scratch_bytes = bytes;
    }
    launch_writer_scaling(g, d_bgr, c->scale_scratch, W, H, c->stream);
    HIPCHK(c, hipGetLastError());
    return POPPY_OK;
}

int seq_add_image(poppy_hip_ctx* c, const uint8_t* d_bgr) {
    uint8_t* dst = seq_next_place(c);
    if (!dst) return fail(c, POPPY_E_STATE, "more frames than the sequence was opened for");
    Timer tm(c, c->stream);
    if (c->timing == 1) tm.mark(nullptr);
    const WriterGeom g = writer_geom(c);
    if (g.scaled()) {
        int rc = scale_into_scratch(c, d_bgr, c->W, c->H, g); if (rc) return rc;
        if (c->timing == 1) tm.mark(scaling_mark(g));
        d_bgr = c->scale_scratch;
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
    if (plane * ring.R > q.idx_bytes) {
        if (q.idx) (void)hipFree(q.idx);
        q.idx = nullptr; q.idx_bytes = 0;
        HIPCHK(c, hipMalloc((void**)&q.idx, plane * ring.R));
        q.idx_bytes = plane * ring.R;
    }
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
        uint8_t* d_idx = q.idx + (size_t)(k % ring.R) * plane;
        Timer tm(c, s);
        if (marks) tm.mark(nullptr);
        launch_pal8_seq_remap(q.store + (size_t)k * q.stride, q.tables, d_idx, W, H, s);
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
    if (each * ring.R > q.gif_bytes) {
        if (q.gif) (void)hipFree(q.gif);
        q.gif = nullptr; q.gif_bytes = 0;
        HIPCHK(c, hipMalloc((void**)&q.gif, each * ring.R));
        q.gif_bytes = each * ring.R;
    }
    if (!q.gif_total) {
        HIPCHK(c, hipHostMalloc((void**)&q.gif_total, 64 * poppy_hip_ctx::kStageRing, hipHostMallocMapped));
        HIPCHK(c, hipHostGetDevicePointer((void**)&q.gif_total_dev, q.gif_total, 0));
    }
    auto d_frame = [&](int k) { return q.gif + (size_t)(k % ring.R) * each; };
    auto total_word = [&](int k) { return (volatile uint32_t*)((uint8_t*)q.gif_total + 64 * (size_t)(k % ring.R)); };
#ifdef POPPY_EXPERIMENTS
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
            uint8_t* d_idx = q.idx + (size_t)(k % ring.R) * (((size_t)W * H + 255) & ~(size_t)255);
            launch_pal8_seq_remap(q.store + (size_t)k * q.stride, q.tables, d_idx, W, H, s);
            if (marks) tm.mark("frame_format");
            launch_gif_lzw(d_idx, d_frame(k) + frame_part, W, H, s);
            if (marks) tm.mark("gif_lzw");
            launch_gif_pack_seq(q.tables, d_frame(k) + frame_part, d_frame(k), (uint32_t*)(q.gif_total_dev + 64 * (size_t)(k % ring.R)), W, H, s);
            if (marks) tm.mark("gif_pack");
        } else
#endif
        enqueue_seq_gif_coding(q.store + (size_t)k * q.stride, q.tables, d_frame(k) + frame_part, d_frame(k), q.gif_total_dev + 64 * (size_t)(k % ring.R), W, H, s, marks ? &tm : nullptr);
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
        if (total < 776 || total > capacity) return fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds");
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
#ifdef POPPY_EXPERIMENTS
    {
        const size_t plane = ((size_t)W * H + 255) & ~(size_t)255;
        if (plane * ring.R > q.idx_bytes) {
            if (q.idx) (void)hipFree(q.idx);
            q.idx = nullptr; q.idx_bytes = 0;
            HIPCHK(c, hipMalloc((void**)&q.idx, plane * ring.R));
            q.idx_bytes = plane * ring.R;
        }
    }
#endif
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
    if (!format_is_coded(c->frame_format)) return seq_hand_over_indices(c, write, user);
    HIPCHK(c, hipStreamSynchronize(c->stream));                   // the ring's streams read the tables
    return seq_hand_over_coded(c, write, user);
}

int seq_finish(poppy_hip_ctx* c, poppy_write_cb write, void* user) {
    if (c->seq.count != c->seq.n) { (void)seq_abort(c); return fail(c, POPPY_E_STATE, "fewer frames than the sequence was opened for"); }
    const int rc = seq_hand_over(c, write, user);
    if (rc) seq_abort_keep_error(c);
    return rc;
}

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

// a PAL8 frame in device memory -> its POPPY_FRAME_GIF frame in `host` (exactly `total` bytes), on the context's stream and waited for: the frames that no slot renders,
// and poppy_hip_pal8_to_gif_frame.  The buffers live for the call.
static int gif_from_device_pal8(poppy_hip_ctx* c, const uint8_t* d_pal8, int W, int H, std::vector<uint8_t>& host) {
    const size_t cap = poppy_frame_bytes(POPPY_FRAME_GIF, W, H);
    uint8_t *work = nullptr, *frame = nullptr;
    hipError_t e = hipMalloc((void**)&work, gif_scratch_bytes(W, H));
    if (e == hipSuccess) e = hipMalloc((void**)&frame, cap + 16);
    uint32_t total = 0;
    if (e == hipSuccess) {
        enqueue_gif_coding(d_pal8, work, frame, nullptr, W, H, c->stream, nullptr, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&total, frame, 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && (total < 776 || total > cap)) { (void)hipFree(work); (void)hipFree(frame); return fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds"); }
    if (e == hipSuccess) { host.resize(total); e = hipMemcpy(host.data(), frame, total, hipMemcpyDeviceToHost); }
    if (work) (void)hipFree(work);
    if (frame) (void)hipFree(frame);
    if (e != hipSuccess) { c->err = std::string("GIF frame coding: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

int download_frame(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, const WriterGeom& g, std::vector<uint8_t>& host, size_t* stride, int n_copies) {
    const int fmt = c->frame_format;
    if (const char* why = format_refuses(fmt, g.w, g.h)) return fail(c, POPPY_E_UNSUPPORTED, why);
    if (g.scaled()) {                                              // scaled first, on the device; everything below is in the writer's geometry
        int rc = scale_into_scratch(c, d_bgr, W, H, g); if (rc) return rc;
        d_bgr = c->scale_scratch; W = g.w; H = g.h;
    }
    if (format_is_sequence(fmt)) {                                 // the copies are the sequence: the host statement on the BGR frame
        std::vector<uint8_t> bgr((size_t)W * H * 3);
        HIPCHK(c, hipMemcpyAsync(bgr.data(), d_bgr, bgr.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        int rc = POPPY_OK;
        const uint8_t* frame = host_frame(c, bgr.data(), (size_t)W * 3, W, H, host, stride, &rc, n_copies);
        return frame ? POPPY_OK : rc;
    }
    *stride = writer_stride(fmt, W);
    const uint8_t* d_frame = d_bgr;
    if (fmt != POPPY_FRAME_BGR) {                                  // converted into the context's scratch: the slots' launches on other buffers
        const bool gif = fmt == POPPY_FRAME_GIF;
        if (format_builds_palette(fmt)) { int rc = alloc_zeroed_tables(c, &c->fmt_scratch_tables, kPal8TableBytes); if (rc) return rc; }
        const size_t bytes = poppy_frame_bytes(gif ? POPPY_FRAME_PAL8 : fmt, W, H);
        if (bytes + 16 > c->fmt_scratch_bytes) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (c->fmt_scratch) (void)hipFree(c->fmt_scratch);
            c->fmt_scratch = nullptr; c->fmt_scratch_bytes = 0;
            HIPCHK(c, hipMalloc((void**)&c->fmt_scratch, bytes + 16));
            c->fmt_scratch_bytes = bytes + 16;
        }
        SlotFormat scratch;
        scratch.i420 = scratch.pal8 = c->fmt_scratch; scratch.pal8_tables = c->fmt_scratch_tables;
        enqueue_conversion(gif ? POPPY_FRAME_PAL8 : fmt, WriterGeom{W, H}, d_bgr, W, H, scratch, c->stream, nullptr, nullptr);
        HIPCHK(c, hipGetLastError());
        if (gif) return gif_from_device_pal8(c, c->fmt_scratch, W, H, host);
        d_frame = c->fmt_scratch;
    }
    host.resize(poppy_frame_bytes(fmt, W, H));
    HIPCHK(c, hipMemcpyAsync(host.data(), d_frame, host.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return POPPY_OK;
}

const uint8_t* host_frame(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, std::vector<uint8_t>& tmp, size_t* out_stride, int* status, int n_copies) {
    const int fmt = c->frame_format;
    *out_stride = stride;
    *status = POPPY_OK;
    if (fmt == POPPY_FRAME_BGR) return bgr;
    if (const char* why = format_refuses(fmt, W, H)) { *status = fail(c, POPPY_E_UNSUPPORTED, why); return nullptr; }
    tmp.resize(poppy_frame_bytes(fmt, W, H));
    std::vector<uint8_t> pal8(format_is_sequence(fmt) && format_is_coded(fmt) ? poppy_frame_bytes(POPPY_FRAME_PAL8_SEQ, W, H) : 0);      // (GIF_SEQ: PAL8_SEQ's frame, then the host coder)
    int rc = format_is_sequence(fmt) ? pal8_seq_of_copies(bgr, stride, std::max(1, n_copies), W, H, pal8.empty() ? tmp.data() : pal8.data()) :
                   fmt == POPPY_FRAME_GIF ? poppy_bgr_to_gif_frame(bgr, stride, W, H, tmp.data()) :
                   fmt == POPPY_FRAME_PAL8 ? poppy_bgr_to_pal8(bgr, stride, W, H, tmp.data()) : poppy_bgr_to_i420(bgr, stride, W, H, tmp.data());
    if (rc == POPPY_OK && !pal8.empty()) rc = poppy_pal8_to_gif_frame(pal8.data(), W, H, tmp.data());
    if (rc) { *status = fail(c, rc, "the frame format refuses this frame"); return nullptr; }
    *out_stride = writer_stride(fmt, W);
    return tmp.data();
}

int write_device_image(poppy_hip_ctx* c, const uint8_t* d_bgr, int W, int H, int n_copies, poppy_write_cb write, void* user) {
    if (const char* why = writer_refuses(c, c->frame_format, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    const WriterGeom g = context_geom(c, W, H);
    std::vector<uint8_t> host; size_t stride = 0;
    int rc = download_frame(c, d_bgr, W, H, g, host, &stride, n_copies); if (rc) return rc;
    for (int j = 0; j < n_copies; ++j) write(user, host.data(), g.w, g.h, stride);
    return POPPY_OK;
}
int write_host_image(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, int n_copies, poppy_write_cb write, void* user) {
    if (const char* why = writer_refuses(c, c->frame_format, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    const WriterGeom g = context_geom(c, W, H);
    std::vector<uint8_t> small, tmp; int rc = POPPY_OK;
    if (g.scaled()) {                                              // the host statement, then the format's as for any host image
        small.resize(poppy_frame_bytes(POPPY_FRAME_BGR, g.w, g.h));
        rc = g.kind == kScaleSize ? poppy_bgr_resize_area(bgr, stride, W, H, g.w, g.h, small.data(), (size_t)g.w * 3)
                                  : poppy_bgr_downscale(bgr, stride, W, H, g.scale, small.data(), (size_t)g.w * 3);
        if (rc) return fail(c, rc, "the frame could not be scaled");
        bgr = small.data(); stride = (size_t)g.w * 3;
    }
    const uint8_t* frame = host_frame(c, bgr, stride, g.w, g.h, tmp, &stride, &rc, n_copies);
    if (!frame) return rc;
    for (int j = 0; j < n_copies; ++j) write(user, frame, g.w, g.h, stride);
    return POPPY_OK;
}

extern "C" {

int poppy_hip_set_frame_format(poppy_hip_ctx* c, int format) {
    if (!c) return POPPY_E_ARG;
    if (!format_known(format)) return fail(c, POPPY_E_ARG, "unknown frame format");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = drain_frames(c); if (rc) return rc; }
    if (c->c1) if (const char* why = writer_refuses(c, format, c->W, c->H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    c->frame_format = format;
    return c->c1 ? alloc_slot_format(c) : POPPY_OK;      // (a pair allocated later gets them in alloc_pair)
}

// A new writer's geometry resizes every buffer of it: the slots' are freed and allocated again, and the captured bodies, which hold their addresses, go.
static int writer_geometry_changed(poppy_hip_ctx* c) {
    if (!c->c1) return POPPY_OK;                                   // (a pair allocated later gets its buffers in alloc_pair)
    for (FrameSlot& f : c->slots) {
        if (f.body) { (void)hipGraphExecDestroy(f.body); f.body = nullptr; }
        free_slot_format_pair(f.fmt);
    }
    return alloc_slot_format(c);
}

int poppy_hip_set_frame_scale(poppy_hip_ctx* c, int factor) {
    if (!c) return POPPY_E_ARG;
    if (factor < 1 || factor > POPPY_FRAME_SCALE_MAX) return fail(c, POPPY_E_ARG, "the frame scale is a whole factor from 1 to 8");
    if (c->seq.open) return fail(c, POPPY_E_STATE, "a sequence is open on this context");
    if (factor > 1 && c->frame_ow) return fail(c, POPPY_E_STATE, "a frame size is set on this context: poppy_hip_set_frame_size(ctx, 0, 0) first");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = drain_frames(c); if (rc) return rc; }
    if (factor == c->frame_scale) return POPPY_OK;
    if (c->c1 && !c->frame_ow) {
        const WriterGeom g = scaled_geom(c->W, c->H, factor);
        if (const char* why = format_refuses(c->frame_format, g.w, g.h)) return fail(c, POPPY_E_UNSUPPORTED, why);
    }
    c->frame_scale = factor;
    return writer_geometry_changed(c);
}

int poppy_hip_set_frame_size(poppy_hip_ctx* c, int ow, int oh) {
    if (!c) return POPPY_E_ARG;
    if (ow < 0 || oh < 0 || (ow == 0) != (oh == 0)) return fail(c, POPPY_E_ARG, "the frame size is two positive numbers, or 0, 0 for none");
    if (c->seq.open) return fail(c, POPPY_E_STATE, "a sequence is open on this context");
    if (ow && c->frame_scale > 1) return fail(c, POPPY_E_STATE, "a frame scale is set on this context: poppy_hip_set_frame_scale(ctx, 1) first");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = drain_frames(c); if (rc) return rc; }
    if (ow == c->frame_ow && oh == c->frame_oh) return POPPY_OK;
    if (c->c1) {
        if (ow && !size_admits(c->W, c->H, ow, oh)) return fail(c, POPPY_E_UNSUPPORTED, kSizeMsg);
        const WriterGeom g = ow ? sized_geom(ow, oh) : scaled_geom(c->W, c->H, c->frame_scale);
        if (const char* why = format_refuses(c->frame_format, g.w, g.h)) return fail(c, POPPY_E_UNSUPPORTED, why);
    }
    c->frame_ow = ow; c->frame_oh = oh;
    return writer_geometry_changed(c);
}

int poppy_hip_bgr_resize_area_form(int W, int H, int ow, int oh) {
    if (W <= 0 || H <= 0 || !size_admits(W, H, ow, oh)) return POPPY_E_ARG;
    return bgr_resize_area_form(W, H, ow, oh);
}

int poppy_hip_bgr_resize_area(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, int ow, int oh, uint8_t* dst, size_t dst_stride) {
    if (!c) return POPPY_E_ARG;
    if (!bgr || !dst || W <= 0 || H <= 0 || !size_admits(W, H, ow, oh) || stride < (size_t)W * 3 || dst_stride < (size_t)ow * 3)
        return fail(c, POPPY_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    // everything lives for the call; the source's place behind a 256-byte boundary is the row pad's low bits (include/poppy_hip.h)
    const size_t row = (size_t)W * 3, shift = (stride - row) % 16, out_row = (size_t)ow * 3;
    uint8_t *d_src = nullptr, *d_dst = nullptr;
    hipError_t e = hipMalloc((void**)&d_src, row * H + shift + 16);
    if (e == hipSuccess) e = hipMalloc((void**)&d_dst, out_row * oh + 16);
    if (e == hipSuccess) e = copy_rows_async(d_src + shift, row, bgr, stride, row, (size_t)H, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch_bgr_resize_area(d_src + shift, d_dst, W, H, ow, oh, c->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = copy_rows_async(dst, dst_stride, d_dst, out_row, out_row, (size_t)oh, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);     // nothing of the call is in flight when its buffers go
    if (e == hipSuccess) e = e_sync;
    for (uint8_t* b : {d_src, d_dst}) if (b) (void)hipFree(b);
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("BGR resize: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

int poppy_hip_bgr_downscale(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H, int factor, uint8_t* dst, size_t dst_stride) {
    if (!c) return POPPY_E_ARG;
    int ow = 0, oh = 0;
    if (!bgr || !dst || poppy_frame_scaled_size(W, H, factor, &ow, &oh) != POPPY_OK || stride < (size_t)W * 3 || dst_stride < (size_t)ow * 3)
        return fail(c, POPPY_E_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    // everything lives for the call; the source's place behind a 256-byte boundary is the row pad's low bits (include/poppy_hip.h)
    const size_t row = (size_t)W * 3, shift = (stride - row) % 16, out_row = (size_t)ow * 3;
    uint8_t *d_src = nullptr, *d_dst = nullptr;
    hipError_t e = hipMalloc((void**)&d_src, row * H + shift + 16);
    if (e == hipSuccess) e = hipMalloc((void**)&d_dst, out_row * oh + 16);
    if (e == hipSuccess) e = copy_rows_async(d_src + shift, row, bgr, stride, row, (size_t)H, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch_bgr_downscale(d_src + shift, d_dst, W, H, factor, c->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = copy_rows_async(dst, dst_stride, d_dst, out_row, out_row, (size_t)oh, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e_sync = hipStreamSynchronize(c->stream);     // nothing of the call is in flight when its buffers go
    if (e == hipSuccess) e = e_sync;
    for (uint8_t* b : {d_src, d_dst}) if (b) (void)hipFree(b);
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("BGR downscale: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

int poppy_hip_pal8_to_gif_frame(poppy_hip_ctx* c, const uint8_t* pal8, int W, int H, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    if (!pal8 || !dst || W <= 0 || H <= 0) return fail(c, POPPY_E_ARG, "bad arguments");
    if (const char* why = format_refuses(POPPY_FRAME_GIF, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = poppy_frame_bytes(POPPY_FRAME_PAL8, W, H);
    uint8_t* d_pal8 = nullptr;
    HIPCHK(c, hipMalloc((void**)&d_pal8, bytes + 16));
    std::vector<uint8_t> host;
    int rc = POPPY_OK;
    if (hipMemcpy(d_pal8, pal8, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = fail(c, POPPY_E_DEVICE, "upload of the PAL8 frame failed");
    if (rc == POPPY_OK) rc = gif_from_device_pal8(c, d_pal8, W, H, host);
    (void)hipFree(d_pal8);
    if (rc == POPPY_OK) memcpy(dst, host.data(), host.size());
    return rc;
}

int poppy_hip_bgr_frames_to_gif_frames(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int W, int H, uint8_t* dst) {
    if (!c) return POPPY_E_ARG;
    if (!bgr || !dst || W <= 0 || H <= 0 || stride < (size_t)W * 3 || n_frames < 1) return fail(c, POPPY_E_ARG, "bad arguments");
    if (const char* why = sequence_refuses(POPPY_FRAME_GIF_SEQ, n_frames, W, H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    if (c->seq.open) return fail(c, POPPY_E_STATE, "a sequence is open on this context");
    HIPCHK(c, hipSetDevice(c->device));
    if (!prepare_pal8()) return fail(c, POPPY_E_DEVICE, "could not raise the palette build's LDS limit");
    // everything lives for the call: the context's own sequence tables, store and rings are not touched
    const size_t row = (size_t)W * 3, place = (row * H + 15) & ~(size_t)15, capacity = poppy_frame_bytes(POPPY_FRAME_GIF_SEQ, W, H);
    uint8_t *store = nullptr, *tables = nullptr, *work = nullptr, *frame = nullptr;
    hipError_t e = hipMalloc((void**)&store, place * (size_t)n_frames);
    if (e == hipSuccess) e = hipMalloc((void**)&tables, kPal8SeqTableBytes);
    if (e == hipSuccess) e = hipMalloc((void**)&work, gif_scratch_bytes(W, H));
    if (e == hipSuccess) e = hipMalloc((void**)&frame, capacity + 16);
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
        if (e == hipSuccess && (total < 776 || total > capacity)) rc = fail(c, POPPY_E_DEVICE, "the coded frame's length is outside its bounds");
        else if (e == hipSuccess) e = hipMemcpy(dst + (size_t)k * capacity, frame, total, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(c->stream);   // nothing of the call is in flight when its buffers go
    for (uint8_t* b : {store, tables, work, frame}) if (b) (void)hipFree(b);
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("GIF sequence coding: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return rc;
}

}  // extern "C"
