// frame_format.cpp — the writer's formats and geometry (frame_format.h) over the formats' records (frame_limits.h): the slots' conversion buffers, the conversion launches and the three setters that
// change this state.  The frame path itself — which stream a frame's conversion runs on, what its completion event rides on, when its copy is issued — is
// frame_render.cpp's and frame_sequence.cpp's (enqueue_body, render_slot, render_sequence_frames).
#include "context.h"

static bool pal8_fits(int W, int H) { return (unsigned long long)W * (unsigned long long)H <= (unsigned long long)POPPY_PAL8_MAX_PIXELS; }
constexpr const char* kPal8SizeMsg = "POPPY_FRAME_PAL8, POPPY_FRAME_PAL8_SEQ, POPPY_FRAME_GIF and POPPY_FRAME_GIF_SEQ take frames of at most 2^24 pixels";
constexpr const char* kGifSizeMsg = "POPPY_FRAME_GIF and POPPY_FRAME_GIF_SEQ take frames of at most 65535 pixels in width and height";
constexpr const char* kJpegSizeMsg = "POPPY_FRAME_JPEG, POPPY_FRAME_JPEG444 and their OPT and SEQ forms take frames of at most 65535 pixels in width and height whose capacity stays below 2^32 bytes";
constexpr const char* kPngSizeMsg = "POPPY_FRAME_PNG, POPPY_FRAME_PNG_RUNS, POPPY_FRAME_PNG_OPT and POPPY_FRAME_PNG_SEQ take frames whose capacity stays below 2^31 bytes";
constexpr const char* kSeqSizeMsg = "POPPY_FRAME_PAL8_SEQ and POPPY_FRAME_GIF_SEQ take sequences of fewer than 2^32 pixels in all";
constexpr const char* kJpegSeqSizeMsg = "POPPY_FRAME_JPEG_SEQ and POPPY_FRAME_JPEG444_SEQ take sequences of at most POPPY_JPEG_SEQ_MAX_SYMBOLS / 64 blocks of 8 x 8 samples in all";
constexpr const char* kPngSeqSizeMsg = "POPPY_FRAME_PNG_SEQ takes sequences of at most POPPY_PNG_SEQ_MAX_SYMBOLS filtered bytes and segments in all";

const char* format_refuses(int fmt, int W, int H) {
    const FormatTraits* t = format_traits(fmt);
    if (!t) return nullptr;
    if (t->raster == kRasterPal8 && !pal8_fits(W, H)) return kPal8SizeMsg;
    if (fits(*t, W, H)) return nullptr;
    return t->coder == kCoderJpeg ? kJpegSizeMsg : t->coder == kCoderPng ? kPngSizeMsg : kGifSizeMsg;
}
const char* sequence_refuses(int fmt, int n, int W, int H) {
    if (const char* why = format_refuses(fmt, W, H)) return why;
    if (const FormatTraits* t = format_traits(fmt)) if (budget_applies(*t)) return nullptr;      // (POPPY_FRAME_JPEG / JPEG444 held back under a sequence budget: 64-bit sums, no limit beyond the frames' own)
    if (const FormatTraits* t = format_traits(fmt)) if (t->coder == kCoderJpeg) return jpeg_seq_fits(n, W, H, t->sampling()) ? nullptr : kJpegSeqSizeMsg;      // the symbol bound; the pixel bound is the palette sequences'
    if (const FormatTraits* t = format_traits(fmt)) if (t->coder == kCoderPng) return png_seq_fits(n, W, H) ? nullptr : kPngSeqSizeMsg;
    return (unsigned long long)n * (unsigned long long)W * (unsigned long long)H >= POPPY_PAL8_SEQ_MAX_PIXELS ? kSeqSizeMsg : nullptr;
}
size_t writer_stride(int fmt, int W) { return format_stride(*format_traits(fmt), W); }
constexpr const char* kSizeMsg = "the frame size set with poppy_hip_set_frame_size takes frames at least as large and at most 8 times as large per side";
WriterGeom scaled_geom(int W, int H, int scale) { return WriterGeom{(W + scale - 1) / scale, (H + scale - 1) / scale, scale, scale > 1 ? kScaleFactor : kScaleNone}; }
WriterGeom sized_geom(int ow, int oh) { return WriterGeom{ow, oh, 1, kScaleSize}; }
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
bool writer_wants_sequence(const poppy_hip_ctx* c, bool has_writer) { return has_writer && writer_traits(c, c->frame_format).sequence; }
// POPPY_FRAME_JPEG and POPPY_FRAME_JPEG444 under a sequence budget: their own records, held back as a sequence
static constexpr FormatTraits kJpegBudgetSeq[2] = {
    {POPPY_FRAME_JPEG,    "JPEG", kRasterI420, kCoderJpeg, poppy_hip::jpeg::k420, false, true, poppy_hip::jpeg::kFrameMinBytes},
    {POPPY_FRAME_JPEG444, "JPEG", kRasterI444, kCoderJpeg, poppy_hip::jpeg::k444, false, true, poppy_hip::jpeg::kFrameMinBytes},
};
const FormatTraits& writer_traits(const poppy_hip_ctx* c, int fmt) {
    const FormatTraits& t = *format_traits(fmt);
    return c->jpeg_seq_budget && budget_applies(t) ? kJpegBudgetSeq[t.sampling() == poppy_hip::jpeg::k444] : t;
}

int alloc_zeroed_tables(poppy_hip_ctx* c, uint8_t** tables, size_t bytes) {
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

int ensure_jpeg_tables(poppy_hip_ctx* c) {
    if (c->jpeg_tables) return POPPY_OK;
    jpeg::QualityTables t;
    jpeg::fill_quality_tables(c->jpeg_quality, &t);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMalloc((void**)&c->jpeg_tables, kJpegTableBytes));
    HIPCHK(c, hipMemcpy(c->jpeg_tables, &t, sizeof t, hipMemcpyHostToDevice));
    return POPPY_OK;
}

bool budget_applies(const FormatTraits& t) { return t.coder == kCoderJpeg && !t.frame_tables; }
constexpr const char* kBudgetFormatMsg = "a JPEG byte budget is set, and the OPT and SEQ forms of the JPEG formats have no budget form: poppy_hip_set_jpeg_budget(ctx, 0) or another format first";
constexpr const char* kSeqBudgetFormatMsg = "a JPEG sequence budget is set, and the OPT and SEQ forms of the JPEG formats have no budget form: poppy_hip_set_jpeg_sequence_budget(ctx, 0) or another format first";
constexpr const char* kTwoBudgetsMsg = "a context has the JPEG byte budget per frame or per sequence, not both: set the other one to 0 first";

// the words behind the 100 tables: the per-frame budget's, then (16 bytes on) the sequence budget's
struct BudgetWords { JpegBudgetParams frame; uint32_t pad[2]; JpegSeqBudgetParams seq; };
static_assert(offsetof(BudgetWords, seq) == 16 && sizeof(BudgetWords) == 32, "the two sets of words, each at an address that stays");
static int write_budget_params(poppy_hip_ctx* c, size_t budget, uint64_t seq_budget, int quality) {
    const BudgetWords p{{(uint32_t)budget, (uint32_t)quality}, {0, 0}, {(uint32_t)seq_budget, (uint32_t)quality, (uint32_t)(seq_budget >> 32), 0}};
    HIPCHK(c, hipMemcpy(c->jpeg_budget_tables + kJpegBudgetTableBytes, &p, sizeof p, hipMemcpyHostToDevice));
    return POPPY_OK;
}
int ensure_jpeg_budget_tables(poppy_hip_ctx* c) {
    if (c->jpeg_budget_tables) return POPPY_OK;
    std::vector<jpeg::QualityTables> all(100);
    for (int q = 1; q <= 100; ++q) jpeg::fill_quality_tables(q, &all[(size_t)q - 1]);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMalloc((void**)&c->jpeg_budget_tables, kJpegBudgetTableBytes + sizeof(BudgetWords)));
    HIPCHK(c, hipMemcpy(c->jpeg_budget_tables, all.data(), kJpegBudgetTableBytes, hipMemcpyHostToDevice));
    return write_budget_params(c, c->jpeg_budget, c->jpeg_seq_budget, c->jpeg_quality);
}
int context_jpeg_seq_budget(poppy_hip_ctx* c, JpegBudget* out) {
    *out = JpegBudget();
    { int rc = ensure_jpeg_budget_tables(c); if (rc) return rc; }
    out->tables = c->jpeg_budget_tables; out->params = c->jpeg_budget_tables + kJpegBudgetTableBytes + offsetof(BudgetWords, seq);
    return POPPY_OK;
}
int context_jpeg_budget(poppy_hip_ctx* c, const FormatTraits& t, JpegBudget* out) {
    *out = JpegBudget();
    if (!c->jpeg_budget || !budget_applies(t)) return POPPY_OK;
    { int rc = ensure_jpeg_budget_tables(c); if (rc) return rc; }
    out->tables = c->jpeg_budget_tables; out->params = c->jpeg_budget_tables + kJpegBudgetTableBytes;
    return POPPY_OK;
}

// the coded frame, the coder's scratch and the pinned length word of a slot: gone (the format they were sized for is another, or the pair's buffers go)
static void free_slot_coded(SlotFormat& f) {
    for (uint8_t* b : {f.coded, f.coded_scratch}) if (b) (void)hipFree(b);
    f.coded = f.coded_scratch = nullptr;
    if (f.coded_total) (void)hipHostFree(f.coded_total);
    f.coded_total = nullptr; f.coded_total_dev = nullptr;
    f.coded_for = POPPY_FRAME_BGR;
}

// the slot's buffer of a raster form (none: none of its own — the BGR frame is the slot's `out` or `scaled`)
static uint8_t* SlotFormat::* const kRasterBuffer[] = {nullptr, &SlotFormat::i420, &SlotFormat::i444, &SlotFormat::pal8};

size_t coding_scratch_bytes(const FormatTraits& t, int W, int H) {
    return t.coder == kCoderJpeg ? jpeg_scratch_bytes(W, H, t.sampling(), t.frame_tables) : t.coder == kCoderPng ? png_scratch_bytes(W, H, t.variant) : gif_scratch_bytes(W, H);
}

// what a coder's scratch holds before its first frame: under JPEG on per-frame tables the frame's symbol counts, zero (the table build leaves them zero again)
hipError_t prepare_coding_scratch(const FormatTraits& t, uint8_t* scratch, int W, int H, hipStream_t s) {
    return t.coder == kCoderJpeg && t.frame_tables ? launch_jpeg_counts_clear(scratch, W, H, t.sampling(), s) : hipSuccess;
}

// What the format's record names, per slot.  A raster step: the buffer of its form, kept until the pair's buffers go, and under PAL8 the conversion's tables.  The
// palette formats, their sequences too: the side stream and its event.  A coder step: the coded frame, the coder's scratch and the pinned length word, sized for
// this format, and under JPEG the context's tables.  A sequence format: the context's sequence tables (a JPEG sequence: its counts and built tables, and the quality's tables) — the store and the index ring depend on the sequence's
// length and, under GIF_SEQ, the ring of coded frames: palette_seq.cpp's seq_begin, seq_finish.  All of it in the writer's geometry; with a scale above 1 or a
// size the scaled BGR frame too.
int alloc_slot_format(poppy_hip_ctx* c) {
    const WriterGeom g = writer_geom(c);
    const int fmt = c->frame_format, W = g.w, H = g.h;
    if (const char* why = writer_refuses(c, fmt, c->W, c->H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    const FormatTraits& t = writer_traits(c, fmt);
    const FrameRaster raster = t.slot_raster();
    for (FrameSlot& slot : c->slots) {
        SlotFormat& f = slot.fmt;
        if (g.scaled() && !f.scaled) HIPCHK(c, hipMalloc((void**)&f.scaled, raster_bytes(kRasterNone, W, H) + 16));
        if (raster != kRasterNone && !(f.*kRasterBuffer[raster])) HIPCHK(c, hipMalloc((void**)&(f.*kRasterBuffer[raster]), raster_bytes(raster, W, H) + 16));
        if (raster == kRasterPal8) { int rc = alloc_zeroed_tables(c, &f.pal8_tables, kPal8TableBytes); if (rc) return rc; }
        if (t.raster == kRasterPal8) { int rc = alloc_slot_side(c, f); if (rc) return rc; }
        if (t.slot_coder() == kCoderNone) continue;                 // (the slot's coded frame: GIF_SEQ codes from the store into the sequence's ring)
        if (t.coder == kCoderJpeg) { int rc = ensure_jpeg_tables(c); if (rc) return rc; f.jpeg_tables = c->jpeg_tables; }
        { int rc = context_jpeg_budget(c, t, &f.jpeg_budget); if (rc) return rc; }
        if (f.coded_for != fmt) free_slot_coded(f);                 // (sized for another coded format; the frames are drained and the bodies of that format are captured again)
        f.coded_for = fmt;
        if (!f.coded) HIPCHK(c, hipMalloc((void**)&f.coded, frame_bytes(t, W, H) + 16));
        if (!f.coded_scratch) {
            HIPCHK(c, hipMalloc((void**)&f.coded_scratch, coding_scratch_bytes(t, W, H)));
            HIPCHK(c, prepare_coding_scratch(t, f.coded_scratch, W, H, nullptr));
            HIPCHK(c, hipStreamSynchronize(nullptr));      // (the frames that use it run on other streams)
        }
        if (!f.coded_total) {
            HIPCHK(c, hipHostMalloc((void**)&f.coded_total, 64, hipHostMallocMapped));
            HIPCHK(c, hipHostGetDevicePointer(&f.coded_total_dev, f.coded_total, 0));
            *f.coded_total = 0;
        }
    }
    if (!t.sequence) return POPPY_OK;
    if (t.coder == kCoderPng) {                                    // a PNG sequence: its summed counts (zero) and its built table
        if (c->seq.png) return POPPY_OK;
        HIPCHK(c, hipMalloc((void**)&c->seq.png, kPngSeqTableBytes));
        HIPCHK(c, hipMemset(c->seq.png, 0, kPngSeqTableBytes));
        return POPPY_OK;
    }
    if (t.coder != kCoderJpeg) return alloc_zeroed_tables(c, &c->seq.tables, kPal8SeqTableBytes);
    if (!t.frame_tables) return ensure_jpeg_budget_tables(c);      // JPEG under a sequence budget: the tables of all qualities and the budget's words (the search's state and lengths: seq_begin)
    { int rc = ensure_jpeg_tables(c); if (rc) return rc; }         // a JPEG sequence: the quality's tables, and the sequence's counts (zero) and built tables
    if (c->seq.jpeg) return POPPY_OK;
    HIPCHK(c, hipMalloc((void**)&c->seq.jpeg, kJpegSeqTableBytes));
    HIPCHK(c, hipMemset(c->seq.jpeg, 0, kJpegSeqTableBytes));
    return POPPY_OK;
}

void free_slot_format_pair(SlotFormat& f) {
    for (uint8_t* b : {f.scaled, f.i420, f.i444, f.pal8, f.pal8_tables}) if (b) (void)hipFree(b);
    f.scaled = f.i420 = f.i444 = f.pal8 = f.pal8_tables = nullptr;
    free_slot_coded(f);
}
void free_slot_format_ctx(SlotFormat& f) {
    if (f.fmt_stream) (void)hipStreamDestroy(f.fmt_stream);
    if (f.bgr_done) (void)hipEventDestroy(f.bgr_done);
}
void free_context_format(poppy_hip_ctx* c) {
    for (DeviceBuffer* b : {&c->scale_scratch, &c->fmt_scratch, &c->seq.store, &c->seq.idx, &c->seq.coded, &c->seq.budget}) b->release();
    for (uint8_t* b : {c->fmt_scratch_tables, c->seq.tables, c->seq.jpeg, c->seq.png, c->jpeg_tables, c->jpeg_budget_tables}) if (b) (void)hipFree(b);
    c->jpeg_tables = c->jpeg_budget_tables = nullptr;
    if (c->seq.coded_total) (void)hipHostFree(c->seq.coded_total);
    c->fmt_scratch_tables = nullptr;
    c->seq = PaletteSeq();
}

bool slot_format_ready(const poppy_hip_ctx* c, const FrameSlot& slot, int fmt, const WriterGeom& g) {
    const SlotFormat& f = slot.fmt;
    const FormatTraits& t = writer_traits(c, fmt);
    const FrameRaster raster = t.slot_raster();
    if (g.scaled() && !f.scaled) return false;
    if (t.sequence && t.coder == kCoderJpeg && !t.frame_tables) return c->seq.open && c->jpeg_budget_tables && c->seq.budget.p;      // (under a sequence budget: the same)
    if (t.sequence && t.coder == kCoderJpeg) return c->seq.open && c->seq.jpeg && c->jpeg_tables;      // (its pass runs on the frame's own stream: enqueue_body)
    if (t.sequence && t.coder == kCoderPng) return c->seq.open && c->seq.png;      // (the same)
    if (t.sequence) return c->seq.open && c->seq.tables && f.fmt_stream && f.bgr_done;
    if (raster != kRasterNone && !(f.*kRasterBuffer[raster])) return false;
    if (raster == kRasterPal8 && !(f.pal8_tables && f.fmt_stream && f.bgr_done)) return false;
    if (t.coder == kCoderJpeg && !f.jpeg_tables) return false;
    return !t.coded() || (f.coded && f.coded_scratch && f.coded_total && f.coded_for == fmt);
}
const uint8_t* slot_bgr(const FrameSlot& f, const WriterGeom& g) { return g.scaled() ? f.fmt.scaled : f.out; }
const uint8_t* slot_frame(const FrameSlot& f, int fmt, const WriterGeom& g) {
    const FormatTraits& t = *format_traits(fmt);
    return t.slot_coder() != kCoderNone ? f.fmt.coded : t.slot_raster() != kRasterNone ? f.fmt.*kRasterBuffer[t.slot_raster()] : slot_bgr(f, g);
}
bool slot_frame_length(const FrameSlot& f, int fmt, size_t capacity, size_t* bytes) {
    const FormatTraits& t = *format_traits(fmt);
    *bytes = t.coded() ? *(volatile uint32_t*)f.fmt.coded_total : capacity;
    return !t.coded() || coded_length_ok(*bytes, capacity, t.least);
}

static void enqueue_gif_coding(const uint8_t* pal8, uint8_t* scratch, uint8_t* frame, void* total_dev, int W, int H, hipStream_t s, hipEvent_t done, Timer* tm) {
    launch_gif_lzw(pal8, scratch, W, H, s);
    if (tm) tm->mark("gif_lzw");
    launch_gif_pack(pal8, scratch, frame, (uint32_t*)total_dev, W, H, s, done);
    if (tm) tm->mark("gif_pack");
}

// (opt: on per-frame tables — the counting pass and the table build in front, both on the coder's scratch, which the slot owns: frames in flight are coded side by side)
// (budget: the search's steps in front, a fixed sequence of dispatches whatever the search finds, then the coder and the gather on the tables it picked)
static void enqueue_jpeg_coding(const uint8_t* planes, const void* tables, uint8_t* scratch, uint8_t* frame, void* total_dev, int W, int H, jpeg::Sampling sm, bool opt, hipStream_t s, hipEvent_t done, Timer* tm,
                                const JpegBudget& budget) {
    if (budget) {
        for (int step = 0; step < kJpegBudgetSteps; ++step) {
            launch_jpeg_measure(planes, budget, scratch, step, W, H, sm, s);
            if (tm) tm->mark("jpeg_measure");
            launch_jpeg_pick(budget, scratch, step, W, H, sm, s);
            if (tm) tm->mark("jpeg_pick");
        }
        launch_jpeg_code_picked(planes, budget, scratch, W, H, sm, s);
        if (tm) tm->mark("jpeg_code");
        launch_jpeg_pack_picked(budget, scratch, frame, (uint32_t*)total_dev, W, H, sm, s, done);
        if (tm) tm->mark("jpeg_pack");
        return;
    }
    if (opt) {
        launch_jpeg_count(planes, tables, scratch, W, H, sm, s);
        if (tm) tm->mark("jpeg_count");
        launch_jpeg_tables(scratch, W, H, sm, s);
        if (tm) tm->mark("jpeg_tables");
    }
    launch_jpeg_code(planes, tables, scratch, W, H, sm, opt, s);
    if (tm) tm->mark("jpeg_code");
    launch_jpeg_pack(tables, scratch, frame, (uint32_t*)total_dev, W, H, sm, opt, s, done);
    if (tm) tm->mark("jpeg_pack");
}

static void enqueue_png_coding(int variant, const uint8_t* bgr, uint8_t* scratch, uint8_t* frame, void* total_dev, int W, int H, hipStream_t s, hipEvent_t done, Timer* tm) {
    launch_png_filter(bgr, scratch, W, H, variant, s);
    if (tm) tm->mark("png_filter");
    launch_png_cost(scratch, W, H, variant, s);
    if (tm) tm->mark("png_cost");
    launch_png_scan(scratch, frame, W, H, variant, s);
    if (tm) tm->mark("png_scan");
    launch_png_pack(scratch, frame, W, H, variant, s);
    if (tm) tm->mark("png_pack");
    launch_png_crc(scratch, frame, W, H, variant, s);
    if (tm) tm->mark("png_crc");
    launch_png_finish(scratch, frame, (uint32_t*)total_dev, W, H, variant, s, done);
    if (tm) tm->mark("png_finish");
}

void enqueue_coding(const FormatTraits& t, const uint8_t* src, const void* tables, uint8_t* scratch, uint8_t* frame, void* total_dev, int W, int H, hipStream_t s, hipEvent_t done, Timer* tm,
                    const JpegBudget& budget) {
    if (t.coder == kCoderGif) enqueue_gif_coding(src, scratch, frame, total_dev, W, H, s, done, tm);
    else if (t.coder == kCoderJpeg) enqueue_jpeg_coding(src, tables, scratch, frame, total_dev, W, H, t.sampling(), t.frame_tables, s, done, tm, budget_applies(t) ? budget : JpegBudget());
    else if (t.coder == kCoderPng) enqueue_png_coding(t.variant, src, scratch, frame, total_dev, W, H, s, done, tm);
}

const uint8_t* enqueue_raster(FrameRaster raster, const uint8_t* src_bgr, int W, int H, const SlotFormat& b, hipStream_t s, hipEvent_t done, Timer* tm) {
    if (raster == kRasterI420) launch_bgr_to_i420(src_bgr, b.i420, W, H, s, done);
    else if (raster == kRasterI444) launch_bgr_to_i444(src_bgr, b.i444, W, H, s, done);
    else {
        // PAL8 is three dispatches, and the palette build in the middle is one workgroup's serial work (about as long as the rest of the frame)
        launch_pal8_hist(src_bgr, b.pal8_tables, W, H, s);
        if (tm) tm->mark("pal8_hist");
        launch_pal8_build(b.pal8_tables, b.pal8, W, H, s);
        if (tm) tm->mark("pal8_build");
        launch_pal8_remap(src_bgr, b.pal8_tables, b.pal8, W, H, s, done);
    }
    if (tm) tm->mark("frame_format");                              // (under PAL8: the index plane alone)
    return b.*kRasterBuffer[raster];
}

void enqueue_conversion(int fmt, const WriterGeom& g, const uint8_t* src_bgr, int W, int H, const SlotFormat& b, hipStream_t s, hipEvent_t done, Timer* tm) {
    const FormatTraits& t = *format_traits(fmt);
    const FrameRaster raster = t.slot_raster();
    const bool codes = t.slot_coder() != kCoderNone;
    if (g.scaled()) {                                              // the conversion's first dispatch; what follows reads the scaled frame
        launch_writer_scaling(g, src_bgr, b.scaled, W, H, s, t.converts() ? nullptr : done);
        if (tm) tm->mark(scaling_mark(g));
        src_bgr = b.scaled; W = g.w; H = g.h;
    }
    const uint8_t* src = src_bgr;                                  // what the coder reads: the raster form, or (PNG) the BGR frame itself
    if (raster != kRasterNone) src = enqueue_raster(raster, src_bgr, W, H, b, s, codes ? nullptr : done, tm);
    if (codes) enqueue_coding(t, src, b.jpeg_tables, b.coded_scratch, b.coded, b.coded_total_dev, W, H, s, done, tm, b.jpeg_budget);
}

extern "C" {

int poppy_hip_set_frame_format(poppy_hip_ctx* c, int format) {
    if (!c) return POPPY_E_ARG;
    if (!format_traits(format)) return fail(c, POPPY_E_ARG, "unknown frame format");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = drain_frames(c); if (rc) return rc; }
    if (c->c1) if (const char* why = writer_refuses(c, format, c->W, c->H)) return fail(c, POPPY_E_UNSUPPORTED, why);
    if (c->jpeg_budget && format_traits(format)->coder == kCoderJpeg && !budget_applies(*format_traits(format))) return fail(c, POPPY_E_UNSUPPORTED, kBudgetFormatMsg);
    if (c->jpeg_seq_budget && format_traits(format)->coder == kCoderJpeg && !budget_applies(*format_traits(format))) return fail(c, POPPY_E_UNSUPPORTED, kSeqBudgetFormatMsg);
    c->frame_format = format;
    return c->c1 ? alloc_slot_format(c) : POPPY_OK;      // (a pair allocated later gets them in alloc_pair)
}

// The quality names the tables that the JPEG kernels read.  They stay where they are — the captured bodies of the slots hold the address — and are rewritten
// once nothing reads them: the frames are drained first.
int poppy_hip_set_jpeg_quality(poppy_hip_ctx* c, int quality) {
    if (!c) return POPPY_E_ARG;
    if (quality < 1 || quality > 100) return fail(c, POPPY_E_ARG, "the JPEG quality is a whole number from 1 to 100");
    if (c->seq.open) return fail(c, POPPY_E_STATE, "a sequence is open on this context");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = drain_frames(c); if (rc) return rc; }
    if (quality == c->jpeg_quality) return POPPY_OK;
    if (c->jpeg_tables) {
        jpeg::QualityTables t;
        jpeg::fill_quality_tables(quality, &t);
        HIPCHK(c, hipMemcpy(c->jpeg_tables, &t, sizeof t, hipMemcpyHostToDevice));
    }
    if (c->jpeg_budget_tables) { int rc = write_budget_params(c, c->jpeg_budget, c->jpeg_seq_budget, quality); if (rc) return rc; }      // (the search's highest quality)
    c->jpeg_quality = quality;
    return POPPY_OK;
}

// The budget is two words that the search's kernels read, at an address that stays: rewritten once nothing reads them.  On and off differ in the dispatches of a
// frame; a slot's captured body records which of the two it holds (FrameSlot::body_budget) and is captured again when the next frame wants the other, whatever
// happened to the format in between (frame_render.cpp: prepare_slot).  Between two positive budgets the bodies stay.
int poppy_hip_set_jpeg_budget(poppy_hip_ctx* c, size_t max_frame_bytes) {
    if (!c) return POPPY_E_ARG;
    if (max_frame_bytes > 0xffffffffull) return fail(c, POPPY_E_ARG, "the JPEG byte budget is at most 2^32 - 1 bytes, or 0 for none");
    if (c->seq.open) return fail(c, POPPY_E_STATE, "a sequence is open on this context");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = drain_frames(c); if (rc) return rc; }
    const FormatTraits& t = *format_traits(c->frame_format);
    if (max_frame_bytes && t.coder == kCoderJpeg && !budget_applies(t)) return fail(c, POPPY_E_UNSUPPORTED, kBudgetFormatMsg);
    if (max_frame_bytes && c->jpeg_seq_budget) return fail(c, POPPY_E_UNSUPPORTED, kTwoBudgetsMsg);
    if (max_frame_bytes == c->jpeg_budget) return POPPY_OK;
    if (c->jpeg_budget_tables) { int rc = write_budget_params(c, max_frame_bytes, c->jpeg_seq_budget, c->jpeg_quality); if (rc) return rc; }
    c->jpeg_budget = max_frame_bytes;
    for (FrameSlot& f : c->slots) {
        int rc = context_jpeg_budget(c, t, &f.fmt.jpeg_budget); if (rc) return rc;
    }
    return POPPY_OK;
}

int poppy_hip_get_jpeg_budget(poppy_hip_ctx* c, size_t* max_frame_bytes) {
    if (!c) return POPPY_E_ARG;
    if (!max_frame_bytes) return fail(c, POPPY_E_ARG, "bad arguments");
    *max_frame_bytes = c->jpeg_budget;
    return POPPY_OK;
}

// The sequence budget is the 64-bit word of JpegSeqBudgetParams that the sequence's pick reads, at an address that stays: rewritten once nothing reads it.  On and
// off differ in who converts a frame — the sequence pass into the store, or the slot's own conversion —: the slots' buffers are allocated for the new state, and a
// slot's captured body, which records the format it converts to (BGR under a sequence), is captured again by the next frame that wants the other.
int poppy_hip_set_jpeg_sequence_budget(poppy_hip_ctx* c, uint64_t max_sequence_bytes) {
    if (!c) return POPPY_E_ARG;
    if (c->seq.open) return fail(c, POPPY_E_STATE, "a sequence is open on this context");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = drain_frames(c); if (rc) return rc; }
    const FormatTraits& t = *format_traits(c->frame_format);
    if (max_sequence_bytes && t.coder == kCoderJpeg && !budget_applies(t)) return fail(c, POPPY_E_UNSUPPORTED, kSeqBudgetFormatMsg);
    if (max_sequence_bytes && c->jpeg_budget) return fail(c, POPPY_E_UNSUPPORTED, kTwoBudgetsMsg);
    if (max_sequence_bytes == c->jpeg_seq_budget) return POPPY_OK;
    if (c->jpeg_budget_tables) { int rc = write_budget_params(c, c->jpeg_budget, max_sequence_bytes, c->jpeg_quality); if (rc) return rc; }
    c->jpeg_seq_budget = max_sequence_bytes;
    return c->c1 ? alloc_slot_format(c) : POPPY_OK;      // (a pair allocated later gets its buffers in alloc_pair)
}

int poppy_hip_get_jpeg_sequence_budget(poppy_hip_ctx* c, uint64_t* max_sequence_bytes) {
    if (!c) return POPPY_E_ARG;
    if (!max_sequence_bytes) return fail(c, POPPY_E_ARG, "bad arguments");
    *max_sequence_bytes = c->jpeg_seq_budget;
    return POPPY_OK;
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

}  // extern "C"
