// context.h — the library's context (one per GPU) and the helpers shared by its translation units:
//   poppy_hip.cpp     context life cycle, HBM layout, plan blob allocation (plan_blob.h), the pair loaders and the C entry points of the resident-pair API
//   frame_render.cpp  one frame (frame_render.h): the frame body and the two halves of a frame, prepare_slot and render_slot
//   frame_sequence.cpp  the multi-frame driver (frame_sequence.h): the planner team's SeqPlans, render_frame, render_sequence and its download pump
//   frame_format.cpp  the writer's formats and geometry (frame_format.h; frame_limits.h: one record per format and the bounds shared with the host statements): slot buffers, conversion launches, the setters
//   palette_seq.cpp   the PAL8_SEQ / GIF_SEQ sequence (palette_seq.h): store, palette, the two hand-over loops;  writer_ring.cpp: the pinned ring towards the writer (writer_ring.h)
//   writer_image.cpp  the frames that no slot renders and the stand-alone conversion entry points (writer_image.h);  writer_buffers.h: the grow-only device buffer and the call-scoped holder
//   pair_begin.cpp    the pair set-up from raw images (pair_begin.h): its schedule and stages, the chain threads (setup_latch.h), the pair_begin entry points
//   pair_setup.cpp    the stage-by-stage entry points of the once-per-pair half: pre-ORB chain, ORB, matching, the RANSAC filter (ransac_fundamental.h), auto-align, tables, margins
//   image_list.cpp    poppy_hip_morph_list;  denoise_hip.cpp: the non-local-means denoise on a context (denoise.h, denoise.cpp: its host statement and weight table)
//   rccl_comm.cpp     the RCCL loader and a context's communicator (rccl_comm.h, comm_guard.h): the two collectives, the abort, the pair state's broadcast, export and import
//   sharded_setup.cpp the pair set-up spread over ranks, as named stages (shard_protocol.h: roles and the keypoint hand-off; local_hub.h: the in-process transport)
//   morph_sharded.cpp one job over N devices;  pool.cpp: pools of contexts, the set-up gate, batches of pairs
//   frame_plan.cpp    host-side planning of a frame;  frame_pal8.cpp, frame_gif.cpp, frame_jpeg.cpp (jpeg_tables.h: the tables it shares with kernels_frame_jpeg.hip), frame_png.cpp, frame_png_runs.cpp and frame_png_opt.cpp (frame_png.h; png_tables.h, png_runs_tables.h and png_opt.h, shared with kernels_frame_png.hip), frame_i444.cpp, frame_scale.cpp, frame_resize.cpp, frame_sink.cpp: the host side of the writer formats, the scaled and resized hand-off and the file sinks
#pragma once
#include "../../include/poppy_hip.h"
#include "foreground.h"
#include "frame_format.h"
#include "palette_seq.h"
#include "writer_image.h"
#include "writer_ring.h"
#include "frame_plan.h"
#include "frame_render.h"
#include "frame_sequence.h"
#include "kernels.h"
#include "kernels_prefilter.h"
#include "orb_detect.h"
#include "point_match.h"
#include "auto_align.h"
#include "comm_guard.h"
#include "pair_state_limits.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>


using namespace poppy_hip;

constexpr int kWarpStampStride = 7;

struct FrameSlot {
    hipStream_t stream = nullptr;        // the stream the slot's independent (phase-mode) frames last ran on: its own, or one of the context's three
    hipStream_t own_stream = nullptr;    // the slot's own (created at its first frame that stays in HBM)
    hipStream_t last_stream = nullptr;   // the stream the frame last rendered here ran on (the context's for chained frames, `stream` otherwise)
    hipEvent_t done = nullptr;           // end of the frame last rendered here
    uint8_t *tr1 = nullptr, *tr2 = nullptr, *out = nullptr;
    float *pyrL = nullptr, *pyrR = nullptr, *pyrM = nullptr, *pyrB = nullptr;
    float *tmp = nullptr, *diff = nullptr;      // only for 1-pixel-wide / -high images (separate unsharp passes)
    float* unsharpF = nullptr;                  // debug copy of the float unsharp result, allocated on demand
    int32_t* triMap = nullptr;
    int map_tag = 0;                            // frame tag of the values last written to triMap (kernels.h: launch_raster); 0 = must be zeroed first
    uint8_t *h_blob = nullptr, *d_blob = nullptr;   // this slot's frame plan (pinned host copy, device copy)
    uint8_t* tile_data = nullptr;                   // the plan's raster expanded on the device: id bytes, record slots, overflow records (kernels_warp_bin.hip)
    void* h_blob_dev = nullptr;                     // device-side address of the pinned copy
    hipEvent_t uploaded = nullptr;                  // the device copy is complete
    hipGraphExec_t body = nullptr;                  // pyrdown .. unsharp of this slot, captured once per pair geometry
    int body_format = POPPY_FRAME_BGR;              // ... with this format's conversion behind the unsharp (re-captured when that changes)
    bool body_budget = false;                       // ... with the JPEG byte budget's search in front of the coder (poppy_hip_set_jpeg_budget: on and off differ in the launches)
    WriterGeom body_geom;                           // ... and this geometry's downscale or resize in front of it (frame_format.h: WriterGeom)
    SlotFormat fmt;                                 // the frame in the writer's format: buffers, side stream and event (frame_format.h)
    hipEvent_t downloaded = nullptr;                // completes when the last download of this slot's `out` towards the writer has read it
    bool dl_pending = false;                        // ... and whether such a download was issued since the slot was last rendered into
    int dl_ring_idx = -1;                           // unless POPPY_HIP_DL_EVENTS is set: the ring stream that carries that download
};

struct poppy_hip_ctx {
    int device = 0;
    poppy_settings cfg;
    hipStream_t stream = nullptr;
    std::string err;

    int W = 0, H = 0;
    bool pair_ready = false;
    // resident buffers
    // c1, c2 and m2 live in ONE allocation behind a small header + point area (PairStateHeader): the "pair state" that a
    // frame needs.  Being contiguous, it travels to other GPUs as a single ncclBroadcast / a single device copy (rccl_comm.cpp).
    uint8_t* arena = nullptr; size_t arena_bytes = 0;
    uint8_t *c1 = nullptr, *c2 = nullptr;
    uint8_t* c2_raw = nullptr;           // image 2 before auto-align (only allocated when auto-align ran): what phase == 1 writes
    bool c2_raw_valid = false;           // ... and whether it belongs to the resident pair
    float *gabor2 = nullptr, *m2 = nullptr;
    std::vector<FrameSlot> slots;        // per-frame working sets, used round-robin
    std::vector<SlotPrep> slot_preps;    // per slot: the frame prepared there (frame_render.h; sized with `slots`)
    unsigned long long frame_seq = 0;    // submit_frame calls so far (a slot prepared ahead names the call it is for)
    std::unique_ptr<SeqPlans> seq_plans; // the plans of a multi-frame call in the making (frame_sequence.h), possibly started ahead by a pair loader; ended by end_seq_plans alone
    // called at the beginning (1) and at the end (0) of every pair set-up from raw images (pair_begin.cpp: pair_begin_impl): a pool's set-up gate (pool.cpp)
    void (*setup_hook)(void* user, poppy_hip_ctx* c, int begin) = nullptr;
    void* setup_hook_user = nullptr;
    bool plan_ahead_credit = true;       // pair loaders start the default sequence's plans (false after a pair whose plans nobody took, until a multi-frame call comes again)
    hipEvent_t inputs_ready = nullptr;   // c1 / c2 / m2 written (recorded on `stream` by the pair loaders)
    const uint8_t* cur1 = nullptr;       // what the next frame warps as "corrected1"
    hipEvent_t cur1_ready = nullptr;     // producer of cur1 when it is a slot's output, else null
    hipStream_t cur1_stream = nullptr;   // ... and the stream that producer ran on
    // Frames that feed on a previous frame all run on `stream`: a cross-stream event on the critical path costs more
    // than the kernels it would overlap.  Frames that read the loaded image run entirely on their slot's stream
    // (created on first use: every extra stream competes for the few hardware queues), so in phase mode several
    // frames are in flight at once.
    int next_slot = 0, last_slot = -1;
    std::vector<PyrLevel> levels;        // 0..pyramid_levels
    void* d_levels = nullptr;            // the tail kernel's tap descriptors (kernels.h: PyrTailPlan), written once per pair geometry
    PyrTailPlan tail;                    // ... and its step table (a kernel argument)
    int first_tail = 1;
    bool use_tail = true;                // false: the coarsest level is too large for one workgroup's LDS (shallow --pyramid): per-level kernels all the way
    // points
    std::vector<P2f> pts1_0, pts1, pts2;
    // per-frame plan blobs (pinned host + device) live in the frame slots, so the host can plan ahead of the GPU
    int max_tris = 0;
    size_t blob_bytes = 0; size_t bins_cap = 0;       // bins_cap: most per-tile triangle-list entries a plan blob has room for
    size_t tile_bytes = 0;                            // size of every slot's tile_data (kernels.h: warp_bin_data_bytes)
    hipStream_t copy_stream = nullptr;
    FramePlan plan;
    OrbDetector orb, orb_b;
    Worker setup_worker;                            // the second image's half of a pair set-up (chain, detector)
    Team planners;                                  // the frame planners of multi-frame calls
    bool writer_attached = false;                   // a multi-frame call with a writer is in progress
    int frame_format = POPPY_FRAME_BGR;             // of the frames handed to writers (poppy_hip_set_frame_format)
    int frame_scale = 1;                            // ... and the whole factor they are scaled down by first (poppy_hip_set_frame_scale; frame_format.h: writer_geom)
    int jpeg_quality = POPPY_JPEG_QUALITY_DEFAULT;  // ... and the quality of the frames of the four JPEG formats (poppy_hip_set_jpeg_quality)
    size_t jpeg_budget = 0;                         // ... the most bytes a POPPY_FRAME_JPEG / JPEG444 frame's file may have (poppy_hip_set_jpeg_budget; 0: off), and what its search reads on
    uint8_t* jpeg_budget_tables = nullptr;          // the device (frame_format.h: context_jpeg_budget)
    uint64_t jpeg_seq_budget = 0;                   // ... or the most bytes the files of a whole sequence of them may have together, at one quality (poppy_hip_set_jpeg_sequence_budget; 0: off; never beside jpeg_budget)
    uint8_t* jpeg_tables = nullptr;                 // ... with its header and quantiser tables on the device (frame_format.h: ensure_jpeg_tables; rewritten in place when the quality changes)
    int frame_ow = 0, frame_oh = 0;                 // ... or the size they are resized to (poppy_hip_set_frame_size; 0, 0: none; never beside a scale above 1)
    DeviceBuffer scale_scratch;                     // the scaled BGR of the copies and fallback frames that no slot renders (writer_image.h: scale_into_scratch)
    DeviceBuffer fmt_scratch;                       // I420 / I444 / PAL8 of the copies and fallback frames that no slot renders (download_frame)
    uint8_t* fmt_scratch_tables = nullptr;          // ... and the PAL8 conversion's tables for them
    PaletteSeq seq;                                 // the sequence formats (PAL8_SEQ, GIF_SEQ, JPEG_SEQ, JPEG444_SEQ, PNG_SEQ): the sequence being collected (palette_seq.h: seq_begin .. seq_finish)
    double wait_ms[4] = {0, 0, 0, 0};               // host waits inside submit_frame since the context was made (POPPY_SEQ_TIMING prints the per-sequence share)
    ForegroundFilter foreground, foreground_b;      // two instances: the images of a pair are filtered side by side
    // The two chain slots (slot 0 = foreground + orb, slot 1 = foreground_b + orb_b; chain_fg / chain_orb below).  After a set-up from raw images the slot
    // chain_b holds the SECOND image's chain state (its detail, its detector's atlas and fetched candidates): poppy_hip_pair_begin_next takes it over in
    // the role of image 1 instead of filtering that image again when kept_gen == chain_gen.  chain_gen moves in every entry point that uses a slot or
    // replaces the resident images (chain_touch), so a state is only reused while nothing else can have changed it.
    int chain_b = 1;
    unsigned long long chain_gen = 1, kept_gen = 0;
    double kept_detail = 0;                         // dft_detail2 of the kept image
    unsigned long long chains_run = 0, chains_reused = 0;      // poppy_hip_chain_counts
    // poppy_hip_morph_list: canvas scratch of the device-side blur_margin (canvas, 32-bit row sums, taps) and the two padded images
    uint8_t* bm_canvas = nullptr; uint32_t* bm_tmp = nullptr; int* bm_taps = nullptr; size_t bm_bytes = 0;
    uint8_t* list_img[2] = {nullptr, nullptr}; size_t list_img_bytes = 0;
    hipStream_t aux_stream = nullptr;
    hipEvent_t setup_ev = nullptr;                  // "the first image's chain has queued its detector's first half" (recorded on `stream` by the first chain's thread when the chains run side by side: gabor2 on copy_stream starts there)
    hipEvent_t c2_up_ev = nullptr;                  // "the second host image is in c2" (recorded on aux_stream by the second chain's thread; gabor2 on copy_stream waits for it)
    double initial_morph_dist = 0;
    int last_nfeatures = 0;
    AutoAligner aligner;
    uint8_t* d_align = nullptr; size_t d_align_bytes = 0;      // staging image of the host-facing align entry points
    unsigned long long n_warp_fast = 0, n_warp_general = 0, n_warp_bin = 0;   // frames by warp kernel since create: tiled (id map), general, fused raster
    // the arguments of the last fused raster + warp launch (poppy_hip_time_last_warp relaunches it)
    struct LastWarp { const float* rec = nullptr; const void* tile_data = nullptr; size_t tile_bytes = 0; const int* toff = nullptr; int tile_w = 0;
                      const uint8_t* c1 = nullptr; const uint8_t* c2 = nullptr; uint8_t* tr1 = nullptr; uint8_t* tr2 = nullptr; WarpExtras ex; bool valid = false; } last_warp;
    int last_descriptor_matches = 0;               // symmetric matches kept by the last pair_begin_descriptors
    // RCCL communicator of this context, or none.  Only rccl_comm.cpp touches it, and hands it to RCCL only inside a CommUse bracket (comm_guard.h) that spans
    // the enqueue call and never the stream synchronise behind it.  morph_sharded's abort path takes the pointer away and waits for the brackets that are open
    // before ncclCommAbort frees the communicator: a late entrant finds none (POPPY_E_STATE), and no thread is inside RCCL with a freed handle — unless a
    // bracket outlasts kCommAbortBoundMs, after which the abort goes ahead regardless and says so in the job's error.  Aborted, the context takes no new
    // communicator until poppy_hip_comm_free.
    CommHandle comm; int comm_rank = 0, comm_world = 1;
    double* d_comm_scratch = nullptr;                               // 8 doubles for the small reductions (rccl_comm.cpp: comm_max_n), allocated with the communicator
    unsigned warp_seq = 0;                      // warp launches issued in timing mode 2 (every kWarpStampStride-th is stamped)
    bool last_warp_fast = false;                   // which warp kernel the last submitted frame used
    bool last_warp_bin = false;
    double last_detail[2] = {0, 0};
    // diagnostics
    bool debug = false;
    bool lazy_mask = false;                     // the level-0 blend kernels compute lbmask from m2; the warp kernel does not write it
    std::vector<int> pyr_forms;                 // the pyramid launches of the last debug-mode frame, (kind, level, arg) triples (poppy_hip_last_pyramid_forms)
    int timing = 0;                      // 0 off, 1 every kernel group (direct launches), 2 the warp kernel only
    struct Mark { const char* name; hipEvent_t ev; };   // name == nullptr opens a frame
    std::vector<Mark> marks; size_t marks_used = 0;
    // staging for host-image entry points
    uint8_t* h_stage = nullptr; size_t h_stage_bytes = 0; void* h_stage_dev = nullptr;
    static const int kStageRing = 8;          // most pinned frames in flight towards the writer (POPPY_HIP_RING, default 3)
    hipStream_t dl_stream = nullptr;
    bool setup_serial = false;                  // pair set-up: the two images' chains one after the other (set by pools of >= 3 contexts per device and by poppy_hip_set_setup_chains)
    hipEvent_t dl_done[kStageRing] = {};
    hipStream_t dl_ring[kStageRing] = {};     // unless POPPY_HIP_DL_EVENTS is set: a stream per pinned ring buffer, carrying nothing but that buffer's copies (no event is recorded behind a copy)
    // (behind everything else: the frame path's members keep the places they had before the filter came)
    // what the RANSAC filter of the last poppy_hip_pair_begin_descriptors_ransac found (poppy_hip_pair_fundamental); set_points of any set-up ends its validity
    struct LastFundamental { bool valid = false; double f[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; int n_matches = 0, n_inliers = 0, best = -1; } fundamental;
    DeviceBuffer ransac_scratch;                    // the filter's points, models and counts on the device (kernels_ransac.hip: ransac_counts_device)
    int max_grid_y = 65535;                         // the device's maxGridSize[1]: the rows one launch_strip_blur takes (blur_margin_rows_fit)
    // the non-local-means denoise (denoise_hip.cpp): the weight table's non-zero prefix on the device with the parameters it was formed for, the staging
    // images of the host-facing entry point and of the list's host images, the list's two denoised images, and poppy_hip_set_denoise's setting (hs 0: off)
    struct Denoise {
        DeviceBuffer table, stage, list_img[2];
        float table_hs = 0; int table_tw = 0, table_sw = 0, L = 0, shift = 0;
        float hs = 0; int tw = 0, sw = 0;
    } denoise;
};

// ---- packed pair state (see poppy_hip_ctx::arena) -------------------------------------------------------------------------
constexpr size_t kPairHeadBytes = 4096;
// (kPairMaxPoints, the point pairs the packed state has room for: pair_state_limits.h)
struct PairStateHeader {
    uint32_t magic, version;
    int32_t W, H, n_points, nfeatures;
    double initial_morph_dist, detail[2];
};
static_assert(sizeof(PairStateHeader) <= kPairHeadBytes, "header area too small");
constexpr uint32_t kPairMagic = 0x50505931u;        // "PPY1"
// nfeatures = int(max_keypoints * 255 / max(d1, d2)) (src/extractor.cpp:40-45).  Where the quotient is no int — both details 0 (two featureless images:
// +inf) or 2^31 and more — C++ leaves the conversion undefined; the reference's x86-64 build converts with cvttsd2si, which gives INT_MIN for every such
// value, and so does this, written out.  The detector's quotas stay in range with it (every quota <= 0: retainBest keeps every candidate).
inline int nfeatures_of(int max_keypoints, double d1, double d2) {
    const double m = std::max(d1, d2);
    const double v = m > 0.0 ? max_keypoints * (255.0 / m) : HUGE_VAL;
    return v >= -2147483648.0 && v < 2147483648.0 ? (int)v : INT32_MIN;
}
inline size_t pair_align(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t pair_state_bytes(int W, int H) {
    const size_t P = (size_t)W * H;
    return kPairHeadBytes + 2 * (size_t)kPairMaxPoints * 8 + 2 * pair_align(P * 3 + 16) + pair_align(P * 4);
}
int drain_frames(poppy_hip_ctx* c);                // waits for every frame queued on this context (all streams)
int stage_pair_state(poppy_hip_ctx* c);            // header + points -> arena head (queued on c->stream)
int adopt_pair_state(poppy_hip_ctx* c);            // arena head -> points, chain state; the pair becomes ready

#define HIPCHK(ctx, call)                                                                             \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                           \
            return POPPY_E_DEVICE;                                                                    \
        }                                                                                             \
    } while (0)

inline int fail(poppy_hip_ctx* c, int code, const char* msg) { c->err = msg; return code; }
inline void set_err(char* err, size_t n, const std::string& s) { if (err && n) snprintf(err, n, "%s", s.c_str()); }      // a caller's error buffer (entry points without a context)
// the pair set-up's dft_detail2 keeps an even number of spectrum rows and columns (include/poppy_hip.h: poppy_hip_pair_begin):
// a frame one pixel wide or high has none, its detail is 0 / 0 — refused before any launch
inline bool setup_size_ok(int W, int H) { return W >= 2 && H >= 2; }
constexpr const char* kSetupSizeMsg = "the pair set-up needs a frame at least 2 x 2 pixels (dft_detail2 of a one-pixel row or column is 0 / 0)";

// shared between the translation units (defined in poppy_hip.cpp)
int alloc_pair(poppy_hip_ctx* c, int W, int H);                                   // resident buffers + frame slots for a W x H pair
int upload_image(poppy_hip_ctx* c, uint8_t* dst, const uint8_t* src, size_t stride, int W, int H);
int set_points(poppy_hip_ctx* c, const float* p1, const float* p2, int n);
int finish_pair_load(poppy_hip_ctx* c);                                           // m2 from gabor2, chain state reset, pair_ready

// Per-kernel timing: events are only RECORDED while frames are queued (no host sync); they are resolved
// in poppy_hip_timing_summary() after the caller has drained the stream.
struct Timer {
    poppy_hip_ctx* c;
    Timer(poppy_hip_ctx* c_, hipStream_t s_) : c(c_), s(s_) {}
    hipStream_t s = nullptr;
    hipEvent_t take(const char* name) {           // next event of the pool, labelled, not recorded
        if (c->marks_used >= c->marks.size()) { hipEvent_t e; (void)hipEventCreate(&e); c->marks.push_back({nullptr, e}); }
        c->marks[c->marks_used].name = name;
        return c->marks[c->marks_used++].ev;
    }
    void mark(const char* name) {
        if (!c->timing) return;
        (void)hipEventRecord(take(name), s);
    }
};

// blur_margin (pair_setup.cpp): the taps, the image's place in the canvas, and canvas -> padded image on the device
constexpr int kBlurMarginTaps = 127;
std::vector<int> blur_margin_taps();
void blur_margin_origin(int W, int H, int UW, int UH, int* x0, int* y0);
bool blur_margin_rows_fit(const poppy_hip_ctx* c, int UH);
constexpr const char* kBlurMarginOffCanvasMsg = "blur_margin: a margin strip leaves the canvas (an image about 99 times as high as wide, or as wide as high; the reference throws there)";
constexpr const char* kBlurMarginRowsMsg = "blur_margin: the canvas has more rows than the device's grid takes in y";
hipError_t blur_margin_strips(const uint8_t* canvas, uint8_t* out, uint32_t* tmp, const int* d_taps, int W, int H, int UW, int UH, hipStream_t s);

// the denoise (denoise_hip.cpp): d_src (rows of `stride` bytes) -> d_dst (tight), queued on the context's stream; the refusals are the caller's
int denoise_queue(poppy_hip_ctx* c, const uint8_t* d_src, size_t stride, uint8_t* d_dst, int w, int h, float hs, int tw, int sw);

inline ForegroundFilter& chain_fg(poppy_hip_ctx* c, int slot) { return slot ? c->foreground_b : c->foreground; }
inline OrbDetector& chain_orb(poppy_hip_ctx* c, int slot) { return slot ? c->orb_b : c->orb; }
inline void chain_touch(poppy_hip_ctx* c) { ++c->chain_gen; }                     // no kept chain state survives this call
