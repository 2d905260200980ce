/* poppy_hip.h — C ABI of the MI355X-native morph hot path (libpoppy_hip.so).
 *
 * Drop-in boundary for kallaballa/Poppy's feature-match -> dense-warp -> blend path.  Every entry
 * point names the reference interface it replaces (paths relative to the reference tree; OCV =
 * third/opencv-4.6.0/modules).  Plain pointers and sizes only; no C++ or torch types cross this line.
 *
 * Conventions
 *   - images are 8-bit BGR, row stride in BYTES given explicitly (cv::Mat::step); float images are
 *     tightly packed; point sets are float pairs (cv::Point2f).
 *   - every function returns POPPY_OK (0) or a negative poppy_status; poppy_hip_last_error(ctx)
 *     returns the message.  Nothing here calls exit() or throws across the boundary (the reference
 *     does: src/poppy.hpp:162,229).
 *   - one ctx per GPU, used from one host thread at a time; different ctx are independent.
 *   - there is NO CPU fallback: without a usable gfx950 device poppy_hip_create() fails.
 *
 * Environment variables (read once per process).  NONE of those the shipped library reads changes a result bit — they choose
 * between forms that the tests hold to the same bytes (tests/test_gpu_prefilter.py::test_setup_alternative_forms_stay_exact,
 * test_gpu_bstage.py::test_unsharp_kernel_forms_on_every_geometry, ::test_pyramid_launch_forms_stay_exact) or print timings:
 *   frames    POPPY_HIP_SLOTS (frames in flight, 4), POPPY_HIP_RING (pinned frames towards the writer, 3), POPPY_HIP_NOGRAPH,
 *             POPPY_HIP_NOFUSE (one launch per small pyramid level), POPPY_HIP_NOCONE (the way up in pairs of levels, as round 5),
 *             POPPY_TAIL_PX, POPPY_TILE_W (64 / 128), POPPY_HIP_IDMAP, POPPY_HIP_GENERALWARP, POPPY_HIP_LBMASK_RIDER,
 *             POPPY_HIP_DL_DEVWAIT, POPPY_HIP_DL_EVENTS (one download stream + an event per frame copy, as until round 5), POPPY_HIP_DONE_PACKET, POPPY_HIP_NO_PREPARE_AHEAD, POPPY_PHASE_OWN_STREAMS, POPPY_UNSHARP_STREAM / _TILE / _ROWS,
 *             POPPY_HIP_WARP_STAMP_STRIDE, POPPY_SEQ_TIMING (stderr)
 *   set-up    POPPY_SETUP_SERIAL, POPPY_GABOR2_FIRST, POPPY_GABOR_DIRECT, POPPY_ACC_STEPS,
 *             POPPY_MED_SETS / _WAVES, POPPY_MED_COLS_MIN / _MIN_HARD / _FORCE / _ROWS, POPPY_ORB_GUESS / _CAP / _KPCAP (test
 *             forms: short lists that must grow), POPPY_SETUP_TIMING (stderr)
 *   several GPUs  POPPY_HIP_RCCL (path of librccl), POPPY_HIP_SHARD_SETUP, POPPY_HIP_SHARD_WORLD1, POPPY_POOL_SETUPS (pair set-ups side by side per device in a pool: 1 from three contexts on), POPPY_POOL_CHAINS
 * Measurement switches that DO change results (parts of a kernel left out, the Gabor transform without its exactness hand-over:
 * POPPY_MED_COLS_SKIP, POPPY_GABOR_NO_REDO, POPPY_GABOR_BAND, POPPY_DL_SKIP_COPY) and the launch-by-launch A/B of wave priorities
 * (POPPY_STAGGER_AB) exist only in a build made with -DPOPPY_EXPERIMENTS (`python -m poppy_amd.build --experiments` writes
 * libpoppy_hip_experiments.so beside the shipped library, never in its place); the shipped library does not read them.
 */
#ifndef POPPY_HIP_H_
#define POPPY_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct poppy_hip_ctx poppy_hip_ctx;

typedef enum {
    POPPY_OK = 0,
    POPPY_E_ARG = -1,        /* bad argument (size mismatch, null pointer, ...)                       */
    POPPY_E_DEVICE = -2,     /* HIP error / no gfx950 device                                           */
    POPPY_E_RANGE = -3,      /* a point fell outside the image where the reference throws StsOutOfRange
                                (OCV/imgproc/src/subdivision2d.cpp:287)                                */
    POPPY_E_STATE = -4,      /* call order violated (e.g. render before pair_begin)                    */
    POPPY_E_NOMATCH = -5,    /* no point pairs: caller should use poppy_hip_dissolve (src/poppy.hpp:125) */
    POPPY_E_UNSUPPORTED = -6 /* stage outside this round's scope (fails loudly, never falls back)      */
} poppy_status;

/* Mirror of poppy::Settings (src/settings.hpp:14-27), passed by value instead of a global singleton. */
typedef struct {
    int number_of_frames;    /* 60  */
    double match_tolerance;  /* 1.0 */
    int max_keypoints;       /* 300 */
    int pyramid_levels;      /* 64  */
    int enable_radial_mask;  /* 0: Extractor::foreground multiplies its mask with draw_radial_gradiant's (src/extractor.cpp:178-197; pinned by restatement only) */
    int enable_auto_align;   /* 0: Matcher::autoAlign on corrected2 and its points before matching (src/matcher.cpp:29-32) */
} poppy_settings;

void poppy_settings_default(poppy_settings* s);

/* ---- lifetime ------------------------------------------------------------------------------ */
poppy_hip_ctx* poppy_hip_create(int device, const poppy_settings* settings);     /* replaces poppy::init, src/poppy.hpp:30-44 */
void poppy_hip_destroy(poppy_hip_ctx* ctx);
const char* poppy_hip_last_error(const poppy_hip_ctx* ctx);
const char* poppy_hip_create_error(void);          /* message of the last failed poppy_hip_create() */

/* ---- per-frame operator (inner boundary) ----------------------------------------------------
 * poppy::morph_images(img1,img2,corrected1,corrected2,gabor2,gf1,gf2,dst,last,morphedPoints,
 *                     srcPoints1,srcPoints2,shapeRatio,maskRatio,linear)   src/algo.hpp:26, src/algo.cpp:178-273
 * Host buffers in, host buffers out, synchronous: this is the parity-test entry point.
 * morphed_pts (n x 2) may be NULL.                                                               */
int poppy_hip_morph_images(poppy_hip_ctx* ctx,
                           const uint8_t* corrected1, size_t stride1,
                           const uint8_t* corrected2, size_t stride2,
                           const float* gabor2_f32x3, int width, int height,
                           const float* src_points1, const float* src_points2, int n_points,
                           double shape_ratio, double mask_ratio,
                           uint8_t* dst, size_t dst_stride, float* morphed_pts);

/* ---- resident pair API (throughput path; frames stay in HBM) ---------------------------------
 * pair_load : uploads corrected1/2 + gabor2 and the matched point sets once per pair
 *             (state that poppy::morph keeps in locals, src/poppy.hpp:114-157).
 * render    : one morph_images step on the resident pair.  chain != 0 reproduces the default CLI
 *             loop body (src/poppy.hpp:177-219): srcPoints1 <- morphedPoints and corrected1 <- frame.
 *             dst may be NULL (frame stays on the device; poppy_hip_frame_device() exposes it).      */
int poppy_hip_pair_load(poppy_hip_ctx* ctx,
                        const uint8_t* corrected1, size_t stride1,
                        const uint8_t* corrected2, size_t stride2,
                        const float* gabor2_f32x3, int width, int height,
                        const float* src_points1, const float* src_points2, int n_points);
/* same, but the three images are already device pointers (tight rows) of this ctx's GPU */
int poppy_hip_pair_load_device(poppy_hip_ctx* ctx, const void* d_corrected1, const void* d_corrected2,
                               const void* d_gabor2_f32x3, int width, int height,
                               const float* src_points1, const float* src_points2, int n_points);
int poppy_hip_render(poppy_hip_ctx* ctx, double shape_ratio, double mask_ratio, int chain,
                     uint8_t* dst, size_t dst_stride);
int poppy_hip_pair_reset(poppy_hip_ctx* ctx);                 /* back to the state right after pair_load */
const void* poppy_hip_frame_device(poppy_hip_ctx* ctx);       /* device pointer of the last frame (u8x3, tight); see poppy_hip_frame_wait */
int poppy_hip_sync(poppy_hip_ctx* ctx);                       /* wait for all queued work of this ctx (every frame stream included) */
void* poppy_hip_stream(poppy_hip_ctx* ctx);                   /* the hipStream_t the pair set-up and CHAINED frames run on */
/* Independent frames (chain == 0, phase mode), several in flight, do not run in the order of poppy_hip_stream(): frames that STAY in HBM
 * (no writer) run on per-slot streams of their own — work queued on poppy_hip_stream() is NOT ordered behind them —; a sequence with a
 * WRITER attached (poppy_hip_render_many / _phases / _morph with a callback) takes the context's own three compute streams in turn, slot
 * index mod 3 — poppy_hip_stream(), the plan-upload stream and the set-up's second stream: the three hardware queues that carry no frame
 * copies —, so work a caller queues on poppy_hip_stream() DURING such a sequence is serialised behind every third frame
 * (POPPY_PHASE_OWN_STREAMS=1: a stream per slot in both cases, the form before round 3).  Either way a caller that renders with
 * dst == NULL and consumes poppy_hip_frame_device() on the device makes its own stream wait for the frame with poppy_hip_frame_wait (a
 * hipStreamWaitEvent on the frame's completion event; stream == NULL: the host waits), or calls poppy_hip_sync().
 * poppy_hip_frame_stream: the stream the last frame was rendered on.  Every pair loader drains all of them first. */
int poppy_hip_frame_wait(poppy_hip_ctx* ctx, void* hip_stream);
void* poppy_hip_frame_stream(poppy_hip_ctx* ctx);

/* Reference frame scheduler (src/poppy.hpp:181-210): shape (= color) ratio of frame j.
 * phase < 0 : default chained mode; 0 <= phase < 1 : phase mode (one frame).                          */
double poppy_frame_ratio(int j, int number_of_frames, double phase);

/* Whole frame loop of poppy::morph on the resident pair (src/poppy.hpp:177-235).  Each finished
 * frame is handed to `write` (the Twriter::write(cv::Mat&) of the reference); the pointer is valid
 * only during the call.  write may be NULL (frames stay on the device: benchmark mode).              */
typedef void (*poppy_write_cb)(void* user, const uint8_t* bgr, int width, int height, size_t stride);
int poppy_hip_morph_frames(poppy_hip_ctx* ctx, double phase, poppy_write_cb write, void* user);
/* The format of the frames handed to a writer.  POPPY_FRAME_BGR (the default): u8x3 rows, stride >= 3 * width.  POPPY_FRAME_I420: planar
 * YUV 4:2:0 as video encoders and Y4M C420jpeg take it, full-range BT.601 with centred chroma, converted on the GPU before the copy to the
 * host (half the bytes of BGR on the link).  Layout of a width x height frame, tight, back to back: Y (width * height bytes), then U,
 * then V (cw * ch bytes each, cw = (width + 1) / 2, ch = (height + 1) / 2).  Y = the Y4M C444 sink's; U, V of each 2 x 2 block, clipped at
 * the right and bottom edges to n = 1, 2 or 4 pixels, k = log2 n, from its channel sums:
 *     U = clamp(((-11059 * sum R - 21709 * sum G + 32768 * sum B + (32768 << k)) >> (16 + k)) + 128, 0, 255)
 *     V = clamp((( 32768 * sum R - 27439 * sum G -  5329 * sum B + (32768 << k)) >> (16 + k)) + 128, 0, 255)   (>> arithmetic)
 * poppy_bgr_to_i420 is the host statement of the format, poppy_frame_bytes its size (0 for an unknown format or an empty frame).
 * poppy_hip_set_frame_format drains the context's frames and applies to every frame handed to a writer by poppy_hip_morph,
 * poppy_hip_morph_frames, poppy_hip_render_many, poppy_hip_render_phases and poppy_hip_morph_list — the phase == 0 / 1 and t == 0 / 1
 * copies and the POPPY_E_NOMATCH linear-blend frames included; under I420 and PAL8 the writer gets (frame, width, height, stride = width), under GIF and JPEG stride = 0.
 * Any other format: POPPY_E_ARG.  These stay BGR whatever the setting: poppy_hip_render / poppy_hip_dissolve into an explicit dst,
 * poppy_hip_frame_device, frames kept on the device (write == NULL), poppy_hip_morph_sharded and poppy_hip_morph_pairs (their contexts
 * are made from poppy_settings), and include/poppy_hip_shim.hpp.  poppy_hip_pool_set_frame_format sets every context of a pool.
 *
 * POPPY_FRAME_PAL8: the frame quantised to 256 colours on the GPU before the copy, for GIF and other palette writers (a third of BGR's
 * bytes on the link).  Layout of a width x height frame: width * height index bytes (tight rows, stride = width), then a 768-byte palette,
 * 256 entries of R, G, B (GIF's order); poppy_frame_bytes = width * height + 768, and the writer gets (frame, width, height, stride =
 * width) with the palette at frame + width * height.  Its value is 8 and POPPY_SINK_GIF is 8 because the values 2 (frame format) and 4
 * (sink) are documented and tested as "unknown format" and stay so; both enums continue from 8.
 * The palette is built per frame, nothing is carried between frames, and there is no dithering.  Integer arithmetic throughout:
 *   1. Histogram.  Cell of a pixel = (R >> 3, G >> 3, B >> 3), 32^3 cells; per cell the pixel count and the sums of the full 8-bit R, G, B.
 *      The sums are 32-bit: a frame of more than POPPY_PAL8_MAX_PIXELS = 2^24 pixels (2^24 * 255 < 2^32) is refused with
 *      POPPY_E_UNSUPPORTED, by poppy_bgr_to_pal8 and by every call that would hand such a frame to a writer under this format.
 *   2. Median cut over the cells.  A box is a cell range [lo, hi] per axis, always shrunk to the bounding box of its occupied cells.  Start
 *      with one box around all occupied cells.  Until there are 256 boxes or no box spans more than one cell: take the box with the largest
 *      count * (longest side in cells) among the boxes that span more than one cell (64-bit product; ties: the lowest box index); cut it
 *      along its longest side (ties: G, then R, then B) at the smallest position k for which the pixels at coordinates <= k are at least
 *      (count + 1) / 2, clamped to k < hi so that both halves are non-empty; the lower half keeps the box's index, the upper half takes
 *      the next free index; both are shrunk.
 *   3. Colours.  Entry i = per channel (sum + count / 2) / count over box i; entries without a box are 0.
 *   4. Indices.  A pixel's index is the box that holds its cell (a table look-up, NOT a nearest-colour search), so every channel of
 *      palette[index] is within 8 * (the box's side) of the pixel, and a frame with at most 256 occupied cells and one colour per cell
 *      comes back exactly.
 * poppy_bgr_to_pal8 is the host statement of all this (dst: poppy_frame_bytes(POPPY_FRAME_PAL8, width, height) bytes).
 *
 * POPPY_FRAME_PAL8_SEQ: PAL8 frames with ONE palette for the whole sequence, so that flat regions of an animation do not shimmer from frame
 * to frame and a GIF can carry a single global colour table (POPPY_SINK_GIF_GLOBAL).  Its value is 16, and POPPY_SINK_GIF_GLOBAL is 16, for
 * the reason PAL8 is 8: 2, 4, 7 and 9 are tested as unknown frame formats and 4 - 7 and 9 as unknown sinks, so both enums go on with 16.
 * A frame has PAL8's layout and size (width * height index bytes, then 768 palette bytes; the writer gets stride = width), every PAL8
 * writer takes it unchanged, and all frames of one sequence carry the same 768 palette bytes.
 *   The rule is steps 1 - 4 above with one change: step 1's histogram is taken over all pixels of ALL frames of the sequence.  Counts and
 *      sums are 64-bit; cuts, tie rules, the (count + 1) / 2 position, shrinking, colours and the table look-up are word for word the
 *      same.  A sequence of one frame therefore gives exactly that frame's PAL8 bytes, and a sequence of n frames gives what PAL8 gives for
 *      the n frames stacked into one width x (n * height) image, cut into n pieces again.
 *   A sequence is the set of frames that one call hands to its writer: one call of poppy_hip_morph (its phase 0 / 1 copies and its
 *      POPPY_E_NOMATCH blend frames included), poppy_hip_morph_frames, poppy_hip_render_many or poppy_hip_render_phases; in
 *      poppy_hip_morph_list, poppy_hip_pool_morph_pairs and poppy_hip_pool_submit_pairs EACH PAIR is one sequence.  The format applies
 *      wherever PAL8 applies and stays BGR wherever PAL8 stays BGR.
 *   Hand-over: the palette is known only after the last frame, so the writer is first called when every frame of the sequence has been
 *      rendered, and then for every frame in order.  Until then the frames wait in device memory, 3 * width * height bytes each, in a buffer
 *      that the context keeps between sequences and grows when needed (an allocation failure is POPPY_E_DEVICE).  If a frame fails to
 *      render, NOTHING of that sequence is written and the call returns the status.
 *   Limits, checked before a frame is rendered or any state changes: a frame has at most POPPY_PAL8_MAX_PIXELS pixels, as under PAL8, and
 *      a sequence has fewer than POPPY_PAL8_SEQ_MAX_PIXELS = 2^32 pixels in all (n_frames * width * height: 2071 frames at 1080p, 517 at
 *      4K), because the device's 3-D prefix sums of the counts are 32-bit words (33^3 of them fill 140 KiB of a compute unit's 160 KiB of
 *      LDS; 64-bit words would not fit).  Both refusals are POPPY_E_UNSUPPORTED.
 * poppy_bgr_frames_to_pal8 is the host statement: n_frames BGR frames, frame k at bgr + k * frame_stride with rows `stride` bytes apart,
 * become n_frames PAL8_SEQ frames back to back in dst (n_frames * poppy_frame_bytes(POPPY_FRAME_PAL8_SEQ, width, height) bytes).  Its
 * refusals are poppy_bgr_to_pal8's, plus n_frames < 1 (POPPY_E_ARG) and the sequence limit; nothing is read or written before them.
 *
 * POPPY_FRAME_GIF: PAL8's per-frame palette and indices with the indices LZW-coded on the GPU and framed as GIF image data, ready to be written behind an
 * image descriptor (POPPY_SINK_GIF_CODED): the LZW coding, 40 ms of one host core per textured 1080p frame in POPPY_SINK_GIF, is off the host.  Its value is 64,
 * and POPPY_SINK_GIF_CODED is 64, because 32 and the values below it are taken or tested as unknown.  Layout of a frame, little-endian:
 *     bytes 0..3     total: the whole frame's length in bytes, these four included (poppy_gif_frame_bytes reads it)
 *     bytes 4..771   the 768-byte palette, exactly PAL8's for this frame
 *     bytes 772..    GIF image data: the minimum-code-size byte 8, the payload in sub-blocks of 255 bytes (a length byte in front of each; the last one
 *                    shorter, none of length 0), then the terminator byte 0
 * The writer gets (frame, width, height, stride = 0): a stride of 0 is how sinks and callers tell a coded frame from a raster, and only `total` bytes are valid.
 *   The payload.  The index plane is one linear run of n = width * height bytes, cut into segments of POPPY_GIF_SEGMENT_PIXELS pixels, the last one shorter.
 *      Every segment is coded by exactly the rule of POPPY_SINK_GIF's coder (codes 0..255 the bytes, 256 clear, 257 end, strings from 258; the width grows
 *      from 9 to 12 bits when the entry just added is the first that needs the next width; a full table is restarted by a clear code): it begins with a clear
 *      code at 9 bits and does not end with an end code but with one clear code at the current width, then the fewest further clear codes at 9 bits (0 to 7;
 *      9 = 1 mod 8) that bring it to a byte boundary.  The segment behind it begins with its own clear code, so clear codes double there.  The last segment
 *      ends with the end code at the current width, padded with zero bits to a byte.  Segments are whole bytes and are concatenated bytewise; repeated clear
 *      codes are ordinary GIF, every decoder takes them.  The segments are independent, which is what lets the GPU code one per wave.
 *   POPPY_GIF_SEGMENT_PIXELS is a constant of the FORMAT: it decides the bytes ("GIF hand-off", has the measurements behind its value).
 *   Capacity.  poppy_frame_bytes(POPPY_FRAME_GIF, w, h) is an upper bound for any content, and the size of the buffers a frame is built in.  A segment of
 *      s <= POPPY_GIF_SEGMENT_PIXELS <= 4096 pixels is: one clear code (9 bits); at most s string codes of at most 12 bits; at most ONE restart clear code
 *      (12 bits: a table fills after 3838 codes, and 2 * 3838 > 4096); the closing clear or end code (at most 12 bits); at most seven padding clear codes
 *      (63 bits) or seven zero bits.  So a segment has at most POPPY_GIF_SEGMENT_BYTES = ceil((9 + 12 * (S + 2) + 63) / 8) bytes, the payload at most P = that
 *      times ceil(n / S), and the frame at most 772 + 1 + P + ceil(P / 255) + 1 bytes.
 *   Limits, refused with POPPY_E_UNSUPPORTED before any state changes: PAL8's 2^24 pixels, and a width or height above 65535 (GIF's 16-bit descriptor).
 * poppy_pal8_to_gif_frame is the host statement (pal8: a PAL8 frame of poppy_frame_bytes(POPPY_FRAME_PAL8, ..) bytes; dst: the capacity), poppy_bgr_to_gif_frame
 * is poppy_bgr_to_pal8 followed by it.  poppy_hip_pal8_to_gif_frame codes a host PAL8 frame on the context's GPU (upload, the two kernels, download of `total`
 * bytes): the same bytes.  The format applies wherever PAL8 applies and stays BGR wherever PAL8 stays BGR.
 *
 * POPPY_FRAME_GIF_SEQ: the coded form of POPPY_FRAME_PAL8_SEQ — ONE palette for the whole sequence and every frame's indices LZW-coded on the GPU, so that a GIF
 * with a single global colour table (POPPY_SINK_GIF_GLOBAL_CODED) is written without any coding on the host.  Its value is 128, and POPPY_SINK_GIF_GLOBAL_CODED is
 * 128: 32, 63 and 65 are tested as unknown formats, 127 and 129 stay unknown.  A frame has POPPY_FRAME_GIF's layout, capacity and limits (poppy_frame_bytes gives
 * the same value for both, poppy_gif_frame_bytes reads both, the writer gets stride = 0).
 *   The rule is the composition of the two above: frame k of a sequence is poppy_pal8_to_gif_frame of frame k of poppy_bgr_frames_to_pal8 over the same frames.
 *      All frames of a sequence therefore carry the same 768 palette bytes, and a sequence of one frame is byte for byte that frame's POPPY_FRAME_GIF.  There is
 *      no delta coding and no transparency: every frame is coded whole.
 *   A sequence and its hand-over are PAL8_SEQ's: one call's frames, each pair in lists and pools; the writer is first called after the last frame has been rendered,
 *      then once per frame in order; nothing is written if a frame fails.  On the device the coder reads each frame's BGR where it waits for the palette, through
 *      the sequence's cell -> index table: the index plane is never stored.
 *   Limits, POPPY_E_UNSUPPORTED before any state changes: PAL8_SEQ's (2^24 pixels per frame, fewer than 2^32 per sequence) and GIF's 65535 per side.
 * poppy_bgr_frames_to_gif_frames is the host statement (poppy_bgr_frames_to_pal8's arguments): frame k goes to dst + k * poppy_frame_bytes(POPPY_FRAME_GIF_SEQ,
 * width, height).  Its refusals are poppy_bgr_frames_to_pal8's plus the 65535 limit; nothing is read or written before them.
 * poppy_hip_bgr_frames_to_gif_frames does the same on the context's GPU (upload into a store that lives for the call, the sequence pass per frame, the palette
 * build, the coder and the gather per frame, download of each frame's `total` bytes): the same bytes.  It needs no resident pair and disturbs none; while the
 * context has a sequence open it returns POPPY_E_STATE.  The format applies wherever PAL8_SEQ applies and stays BGR wherever PAL8_SEQ stays BGR.
 *
 * POPPY_FRAME_JPEG: the frame coded on the GPU as one baseline JPEG (JFIF) file, ready to be written into a Motion-JPEG AVI (POPPY_SINK_MJPEG) or to disk as it
 * is: 24-bit colour, and a fraction of I420's bytes on the link.  Its value is 256, and POPPY_SINK_MJPEG is 256; 255 and 257 stay unknown.  Layout, little-endian:
 *     bytes 0..3     total: the whole frame's length in bytes, these four included (poppy_jpeg_frame_bytes reads it)
 *     bytes 4..      one complete JFIF file, FF D8 .. FF D9
 * The writer gets (frame, width, height, stride = 0), as under GIF, and only `total` bytes are valid.  The rule is integer arithmetic throughout, 32-bit, all
 * shifts arithmetic, all divisions of non-negative numbers; two implementations agree byte for byte.
 *   Planes.  The frame's I420 planes exactly as poppy_bgr_to_i420 gives them: Y is w x h, U (Cb) and V (Cr) are cw x ch.
 *   MCUs.  One MCU is 16 x 16 luma samples, six 8 x 8 blocks in the order Y00, Y01 (right), Y10 (below), Y11, Cb, Cr; ceil(w / 16) x ceil(h / 16) MCUs in raster
 *      order.  MCU (mx, my)'s luma blocks begin at sample (16 mx + 8 i, 16 my + 8 j), its chroma blocks at (8 mx, 8 my) of their planes.  A sample outside its
 *      plane is the nearest one inside: x clamped to the plane's width - 1, y to its height - 1.
 *   FDCT.  s(x, y) = sample - 128.  K = {8192, 8035, 7568, 6811, 5793, 4551, 3135, 1598}, K[k] = round(8192 cos(k pi / 16)).  The 8 x 8 table T has
 *      T[0][x] = 5793 and, for u > 0, T[u][x] = +-K[..] = round(8192 cos((2 x + 1) u pi / 16)) (so T[u][x] = round(2^14 a(u) cos(..)) for the orthonormal
 *      DCT's a(0) = sqrt(1 / 8), a(u) = 1 / 2).  Two passes, rows first:
 *         t(y, u) = (sum over x of T[u][x] * s(x, y) + 1024) >> 11
 *         F(v, u) = (sum over y of T[v][y] * t(y, u) + 8192) >> 14
 *      F is 8 times the orthonormal DCT coefficient (three fractional bits, as libjpeg's integer transforms leave them).  |sum| stays below 2^28 in both passes.
 *   Quantisation.  The Annex K base tables of ITU-T T.81 (K.1 for Y, K.2 for Cb and Cr), scaled by libjpeg's rule: for a quality q from 1 to 100,
 *      scale = 5000 / q below 50 and 200 - 2 q from 50 up, Q = clamp((base * scale + 50) / 100, 1, 255).  The divisor takes in the transform's factor 8, and the
 *      division rounds half away from zero: m = (|F| + 4 Q) / (8 Q), the quantised coefficient is m with F's sign.  It is within 1 of a double-precision DCT's
 *      coefficient quantised by the same Q (ITU-T T.83's bar).  A DC coefficient lies in -1024 .. 1016, an AC coefficient's magnitude below 1024.
 *   Huffman coding.  Baseline sequential, the four "typical" tables of Annex K.3 (K.3 and K.5 for Y, K.4 and K.6 for Cb and Cr), never optimised.  Per block: the
 *      DC difference to the previous block of the same component in the segment (the first: to 0) as its category's code and the category's low bits (a negative
 *      value v as v - 1); then the AC coefficients in zig-zag order as run / category symbols, ZRL (F0) for every 16 zeros in front of a non-zero coefficient,
 *      EOB (00) when the block ends in zeros, nothing when coefficient 63 is non-zero.  Bits are packed most significant first.
 *   Restart intervals.  The MCU sequence is cut into segments of POPPY_JPEG_RESTART_MCUS MCUs, whatever the row; the last may be shorter.  Every segment begins
 *      with DC predictors of 0, is padded with 1-bits to a byte boundary and byte-stuffed (FF -> FF 00).  Segment k, unless it is the last, is followed by
 *      RST(k mod 8) = FF D0 + (k mod 8); EOI follows the last.  Segments are whole bytes and independent, which is what lets the GPU code one per wave.
 *      POPPY_JPEG_RESTART_MCUS is a constant of the FORMAT: it decides the bytes ("JPEG hand-off", has what stands behind its value).
 *   Header.  613 bytes, so the entropy-coded data begins at frame offset 617: SOI; APP0 "JFIF" 1.01, units 0, density 1 : 1, no thumbnail; ONE DQT with table 0
 *      and table 1 (8-bit entries, zig-zag order); SOF0 with 8-bit precision, the true height and width, components 1 (2 x 2, table 0), 2 and 3 (1 x 1, table 1);
 *      ONE DHT with DC 0, AC 0, DC 1, AC 1; DRI with the interval (always present); SOS with components 1 (tables 0 / 0), 2 and 3 (1 / 1), Ss 0, Se 63, Ah / Al 0.
 *   Capacity.  poppy_frame_bytes(POPPY_FRAME_JPEG, w, h) is an upper bound for any content at any quality, and the size of the buffers a frame is built in.  A block
 *      is at most a DC code of 11 bits (table K.4's longest; K.3's is 9) with 11 value bits (the differences' range is 2040 < 2^11) and 63 AC codes of 16 bits with 10 value bits: 1660 bits.  A
 *      coefficient in front of which ZRL symbols stand costs less than that many coefficients coded singly (a ZRL is 11 or 10 bits for 16 coefficients), and EOB
 *      only ever replaces coefficients.  A segment of R = POPPY_JPEG_RESTART_MCUS MCUs is at most ceil(6 * 1660 * R / 8) bytes with its padding, twice that when
 *      every byte is stuffed, and 2 bytes of marker: POPPY_JPEG_SEGMENT_BYTES.  The frame is at most 617 + ceil(MCUs / R) * POPPY_JPEG_SEGMENT_BYTES bytes (about
 *      9.7 bytes per pixel: the price of a bound that holds for noise at quality 100 with every byte FF).
 *   Limits, refused with POPPY_E_UNSUPPORTED before any state changes: a width or height above 65535 (SOF0's 16 bits), and a capacity of 2^32 bytes or more
 *      (`total` is 32 bits; about 440 million pixels).
 * poppy_i420_to_jpeg_frame is the host statement (i420: poppy_frame_bytes(POPPY_FRAME_I420, ..) bytes; dst: the capacity; POPPY_E_ARG for a null pointer, an empty
 * frame or a quality outside 1..100), poppy_bgr_to_jpeg_frame is poppy_bgr_to_i420 followed by it.  poppy_hip_i420_to_jpeg_frame codes a host I420 frame on the
 * context's GPU at the given quality (upload, the two kernels, download of `total` bytes): the same bytes; it needs no resident pair and disturbs none.
 * poppy_hip_set_jpeg_quality sets the quality of the frames a context hands to its writers (POPPY_JPEG_QUALITY_DEFAULT = 90 until then): POPPY_E_ARG outside
 * 1..100, POPPY_E_STATE while a sequence is open; it drains the context's frames, as poppy_hip_set_frame_format does, and takes effect whatever the format is at
 * the time.  poppy_hip_pool_set_jpeg_quality sets every context of a pool (POPPY_E_STATE with work submitted).
 * The format applies wherever GIF applies — poppy_hip_morph, poppy_hip_morph_frames, poppy_hip_render_many, poppy_hip_render_phases, poppy_hip_morph_list and
 * pools, the phase 0 / 1 and t == 0 / 1 copies and the POPPY_E_NOMATCH frames included, under poppy_hip_set_frame_scale and poppy_hip_set_frame_size the host
 * statement at the writer's geometry — and stays BGR wherever GIF stays BGR.  There is no 4:2:2 sampling, no progressive mode and no sequence form.
 *
 * POPPY_FRAME_JPEG444: POPPY_FRAME_JPEG with full-resolution chroma (4:4:4), for texture and saturated edges, where it is 4:2:0 that costs the quality and not
 * the quantiser; about 1.3 times JPEG's bytes.  Its value is 512; 511 and 513 stay unknown, and there is no sink value of its own: POPPY_SINK_MJPEG takes its
 * frames.  The layout is JPEG's (`total`, then one complete JFIF file), the writer gets stride = 0, poppy_jpeg_frame_bytes reads `total`, and the rule is
 * POPPY_FRAME_JPEG's word for word with these changes only:
 *   Planes.  The frame's I444 planes exactly as poppy_bgr_to_i444 gives them: three tight w x h planes back to back, Y, then U (Cb), then V (Cr).  Y is I420's Y;
 *      U and V are I420's formulas with n = 1, k = 0, per pixel and with arithmetic shifts:
 *         U = clamp(((-11059 R - 21709 G + 32768 B + 32768) >> 16) + 128, 0, 255)
 *         V = clamp((( 32768 R - 27439 G -  5329 B + 32768) >> 16) + 128, 0, 255)
 *      (pure blue gives U = 256 before the clamp).  These are the planes POPPY_SINK_Y4M writes.  I444 is a statement and a kernel, not a hand-off format: it
 *      saves nothing on the link against BGR.
 *   MCUs.  One MCU is 8 x 8 samples, three 8 x 8 blocks in the order Y, Cb, Cr; ceil(w / 8) x ceil(h / 8) MCUs in raster order.  Every block of MCU (mx, my)
 *      begins at sample (8 mx, 8 my) of its plane.  A sample outside the plane is the nearest one inside, as under JPEG.
 *   FDCT, quantisation, Huffman coding.  Unchanged: the same T and shifts, the Annex K tables at the context's quality, m = (|F| + 4 Q) / (8 Q), the typical
 *      Huffman tables — table 0 for Y, table 1 for Cb and Cr — and one DC predictor per component.
 *   Restart intervals.  POPPY_JPEG444_RESTART_MCUS = 16 MCUs, a constant of the format: 16 x 3 = 48 blocks, JPEG's 8 x 6, so POPPY_JPEG_SEGMENT_BYTES bounds a
 *      segment of this format too.
 *   Header.  613 bytes, the entropy-coded data begins at frame offset 617.  It is JPEG's header for the same size and quality except in exactly two bytes: SOF0
 *      component 1's sampling byte is 0x11 (1 x 1) instead of 0x22, and DRI's low byte is 16 instead of 8.
 *   Capacity.  poppy_frame_bytes(POPPY_FRAME_JPEG444, w, h) = 617 + ceil(MCUs / 16) * POPPY_JPEG_SEGMENT_BYTES: about 19.5 bytes per pixel, twice JPEG's, because
 *      there are twice the blocks.
 *   Limits, refused with POPPY_E_UNSUPPORTED before any state changes: a width or height above 65535, and a capacity of 2^32 bytes or more (about 220 million
 *      pixels).
 * poppy_bgr_to_i444 is the host statement of the planes (dst: 3 * width * height bytes; POPPY_E_ARG for a null pointer, an empty frame or stride < 3 * width),
 * poppy_hip_bgr_to_i444 does the same on the context's GPU (upload, the kernel, download): the same bytes; it needs no resident pair and disturbs none.  As with
 * poppy_hip_bgr_downscale, the device copy of the source is tight and begins (stride - 3 * width) mod 16 bytes behind a 256-byte boundary.
 * poppy_i444_to_jpeg_frame is the host statement of the format (i444: 3 * width * height bytes; dst: the capacity), poppy_bgr_to_jpeg444_frame is
 * poppy_bgr_to_i444 followed by it; both refuse what poppy_i420_to_jpeg_frame and poppy_bgr_to_jpeg_frame refuse.  poppy_hip_i444_to_jpeg_frame codes a host I444
 * frame on the context's GPU at the given quality (upload, the two kernels, download of `total` bytes): the same bytes; no resident pair needed, none disturbed.
 * poppy_hip_set_jpeg_quality and poppy_hip_pool_set_jpeg_quality serve both formats.  The format applies wherever JPEG applies, under poppy_hip_set_frame_scale
 * and poppy_hip_set_frame_size as the host statement at the writer's geometry, and stays BGR wherever JPEG stays BGR.
 *
 * POPPY_FRAME_JPEG_OPT (4096) and POPPY_FRAME_JPEG444_OPT (8192): POPPY_FRAME_JPEG and POPPY_FRAME_JPEG444 on Huffman tables built from the frame's own symbols
 * instead of the Annex K examples: the same planes, quality, quantisation, sampling, restart intervals and coefficients, so a file decodes to exactly the pixels of
 * the JPEG / JPEG444 file of the same frame, in fewer bytes (about 0.8 to 0.95 of them; DESIGN.md section 4, "JPEG optimised-table hand-off").  4095, 4097, 8191
 * and 8193 stay unknown; there is no sink value: POPPY_SINK_MJPEG takes the frames.  Layout and writer call are JPEG's, poppy_jpeg_frame_bytes reads `total`.  The
 * rule is the other format's word for word except for the tables, the DHT segment that names them and what follows from their sizes:
 *   Counts.  Four tables: DC 0, AC 0 (Y), DC 1, AC 1 (Cb and Cr).  count[s] is how often the POPPY_FRAME_JPEG coder emits symbol s from that table for this frame:
 *      a DC category 0..11, an AC run / size byte, F0 once per ZRL, 00 once per EOB.  Every table of every frame has at least one symbol (every block has a DC
 *      symbol, and every frame has blocks of both tables' components; a block without an AC symbol ends in coefficient 63, which is an AC symbol).
 *   Table rule.  poppy_jpeg_optimal_table(counts[256], bits[16], vals[256], &n) is T.81 Annex K.2 as libjpeg's jpeg_gen_optimal_table words it, with every tie
 *      decided; host only, integers only (sums in 64 bits):
 *      1. freq[0..255] = counts, freq[256] = 1: the reserved entry, which keeps any real code from being all ones.  Every entry is its own tree.
 *      2. Repeat: c1 is the index of the smallest non-zero freq, the LARGEST index among equals; c2 the same among the other entries; stop when there is no c2.
 *         freq[c1] += freq[c2], freq[c2] = 0; every symbol in c1's tree and in c2's tree gets one bit longer; c2's tree joins c1's.
 *      3. Count the symbols of each length, the reserved entry among them.  A length may reach 256 (257 leaves); the array holds that.
 *      4. Annex K.3, for i from the longest length down to 17: while bits[i] > 0, set j = i - 2 and step j down until bits[j] > 0; then bits[i] -= 2,
 *         bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1.
 *      5. Take one away from the longest non-empty length <= 16: the reserved entry's code.
 *      6. vals is the symbols that have a count, ordered by their length BEFORE step 4, then by symbol value; n is their number.
 *      Codes are canonical: in the order of vals, the first code of length 1 is 0, a code is its predecessor plus 1, shifted left by the difference in length.
 *      POPPY_E_ARG for a null pointer, for counts that are all zero, and for a sum of 2^32 - 1 or more (with the reserved entry the root's count would not fit
 *      32 bits).  poppy_hip_jpeg_optimal_table runs the device's table build alone on one table's counts and gives the same bits, vals and n.
 *   Count bound.  A frame the format accepts has a capacity below 2^32 bytes, so fewer than 2^32 / POPPY_JPEG_OPT_SEGMENT_BYTES < 215500 segments of 48 blocks,
 *      fewer than 10.4 million blocks, each with one DC symbol and at most 63 AC symbols: a table's sum stays below 6.6 * 10^8 < 2^30, far below the limit, and
 *      the device adds and merges in 32 bits.
 *   Header.  POPPY_FRAME_JPEG's (JPEG444's) header byte for byte up to the DHT marker at file offset 173; then ONE DHT segment, FF C4, its length
 *      2 + sum(17 + n), and per table in the order DC 0, AC 0, DC 1, AC 1 the class / id byte (00, 10, 01, 11), bits[16] and the n values; then DRI and SOS as
 *      before.  The header is 197 + sum(17 + n) bytes — at most 613, since a DC table has at most 12 symbols and an AC table at most 162 — and the
 *      entropy-coded data begins right behind it, at frame offset 4 + that: no longer a constant.
 *   Capacity.  A code has at most 16 bits after step 4, and a DC tree has at most 13 leaves (12 categories and the reserved entry), so a DC code has at most 12
 *      bits where table K.4 stops at 11.  A block is at most 12 + 11 + 63 * (16 + 10) = 1661 bits (ZRL and EOB cost no more than under JPEG: a ZRL is one code of
 *      at most 16 bits for 16 coefficients), a segment at most ceil(48 * 1661 / 8) bytes, twice that stuffed, and 2 bytes of marker:
 *      POPPY_JPEG_OPT_SEGMENT_BYTES = 19934.  poppy_frame_bytes = 4 + 613 + segments * POPPY_JPEG_OPT_SEGMENT_BYTES, with JPEG's (JPEG444's) number of segments.
 *      The smallest frame is the header with four one-symbol tables, one byte of data and EOI: 4 + 197 + 4 * 18 + 1 + 2 = 276 bytes.
 *   Limits.  JPEG's: a side above 65535 or a capacity of 2^32 bytes or more is POPPY_E_UNSUPPORTED.
 * poppy_i420_to_jpeg_opt_frame and poppy_i444_to_jpeg_opt_frame are the host statements (two passes over the same coefficients: count, build, code; arguments and
 * refusals as poppy_i420_to_jpeg_frame's, dst: the capacity), poppy_bgr_to_jpeg_opt_frame and poppy_bgr_to_jpeg444_opt_frame the conversion followed by them.
 * poppy_hip_i420_to_jpeg_opt_frame and poppy_hip_i444_to_jpeg_opt_frame code host planes on the context's GPU (upload, four kernels — count, table build, code,
 * gather —, download of `total` bytes): the same bytes.  poppy_hip_set_jpeg_quality serves these formats too, and they apply wherever JPEG applies, under
 * poppy_hip_set_frame_scale and poppy_hip_set_frame_size as the host statement at the writer's geometry, and stay BGR wherever JPEG stays BGR.
 *
 * POPPY_FRAME_JPEG_SEQ (32768) and POPPY_FRAME_JPEG444_SEQ (65536): POPPY_FRAME_JPEG_OPT and POPPY_FRAME_JPEG444_OPT on ONE set of four Huffman tables for all
 * the frames a call hands to its writer, as POPPY_FRAME_PAL8_SEQ is PAL8 on one palette: one table build per sequence instead of one per frame.  32767, 32769,
 * 65535 and 65537 stay unknown in both enums; there is no sink value of their own: POPPY_SINK_MJPEG takes the frames.  Layout and writer call are JPEG_OPT's,
 * poppy_jpeg_frame_bytes reads `total`.  The rule is POPPY_FRAME_JPEG_OPT (JPEG444_OPT) word for word, except:
 *   Counts.  The four count tables (DC 0, AC 0, DC 1, AC 1) are the element-wise sums, over all frames of the sequence, of the counts POPPY_FRAME_JPEG_OPT
 *      defines for each frame.  One call of the unchanged table rule (poppy_jpeg_optimal_table) per table gives the sequence's tables.  A symbol that some
 *      frame never emits still has a code, because another frame gave it a count; a symbol no frame emits has none.
 *   Frames.  Every frame is a complete baseline JFIF file in JPEG_OPT's layout — `total`, the header with ONE DHT segment naming the four tables, DRI, SOS, the
 *      restart intervals, EOI — and stands alone, so that MJPEG players open it.  All frames of a sequence carry the same header bytes: width, height, quality,
 *      DHT and so the data's offset are identical.  A sequence of one frame is byte for byte that frame's POPPY_FRAME_JPEG_OPT (JPEG444_OPT) frame, and every
 *      frame decodes to exactly the pixels of its POPPY_FRAME_JPEG (JPEG444) frame.
 *   Capacity, least, stride.  JPEG_OPT's: the derivation uses only "a code has at most 16 bits, a DC code at most 12", which holds for any counts.
 *      poppy_frame_bytes(POPPY_FRAME_JPEG_SEQ, w, h) = poppy_frame_bytes(POPPY_FRAME_JPEG_OPT, w, h), the smallest frame has 276 bytes, the writer is told stride 0.
 *   Limits.  Checked on the arguments alone, before any state changes, and refused with POPPY_E_UNSUPPORTED: JPEG_OPT's per frame; and for the sequence, with B
 *      the number of 8 x 8 blocks of a frame over all components in the format's sampling (MCUs x 6 in 4:2:0, MCUs x 3 in 4:4:4), n_frames * B * 64 <=
 *      POPPY_JPEG_SEQ_MAX_SYMBOLS = 2^32 - 2.  A block has at most 64 symbols, so every table's sum then stays below the table rule's own refusal and the device
 *      keeps adding and merging in 32 bits.  That allows 1370 frames at 1080p in 4:2:0.
 *   A sequence is exactly what it is under POPPY_FRAME_PAL8_SEQ: all frames one call hands to its writer — one pair's frames in poppy_hip_morph_list and in the
 *      pool; the t = 0 / t = 1 copies of poppy_hip_render_phases and the phase-0 / phase-1 short-circuits (N copies of one image: its counts N times) count
 *      among them.  The writer is first called after the last frame is rendered, and gets the frames in order.
 * poppy_i420_frames_to_jpeg_seq_frames and poppy_i444_frames_to_jpeg_seq_frames are the host statements: n_frames frames of planes, frame k at planes +
 * k * frame_stride, in three passes over the same coefficients — every frame counted into the sums, one build, every frame coded; frame k goes to dst +
 * k * poppy_frame_bytes(format, width, height).  poppy_bgr_frames_to_jpeg_seq_frames and poppy_bgr_frames_to_jpeg444_seq_frames take poppy_bgr_frames_to_pal8's
 * arguments and the quality, and are the conversion of every frame followed by them.  POPPY_E_ARG for a null pointer, n_frames < 1, an empty frame, a row stride
 * below 3 * width, a frame_stride shorter than a frame (the planes' bytes; stride * (height - 1) + 3 * width) and a quality outside 1..100; POPPY_E_UNSUPPORTED
 * for the limits; both before a byte is read.  poppy_hip_bgr_frames_to_jpeg_seq_frames and poppy_hip_bgr_frames_to_jpeg444_seq_frames do the same on the
 * context's GPU, on a sequence that lives for the call (per frame: upload, raster kernel, counting kernel; one table build; per frame: coder, gather, download of
 * `total` bytes): the same bytes; they need no resident pair and disturb neither one nor the context's own sequence.  poppy_hip_set_jpeg_quality serves these
 * formats, poppy_hip_pool_set_frame_format takes them, and they apply wherever POPPY_FRAME_JPEG applies, under poppy_hip_set_frame_scale and
 * poppy_hip_set_frame_size as the host statement at the writer's geometry (the tables are taken over the SCALED frames), and stay BGR wherever JPEG stays BGR
 * (poppy_hip_morph_sharded, poppy_hip_morph_pairs).
 *
 * JPEG byte budget: POPPY_FRAME_JPEG and POPPY_FRAME_JPEG444 frames of at most B bytes each, for a stream with a bitrate cap, a slot in a ring or a file that must
 * stay under a size.  poppy_hip_set_jpeg_budget(ctx, B) sets it, 0 (the default) is off and leaves every frame, byte and launch as it is without; with B > 0 the
 * context's quality (poppy_hip_set_jpeg_quality) is the HIGHEST quality a frame may have, and every frame is coded at the quality this rule picks for it:
 *   Size.  size(q) is the length of the JFIF file of the frame's POPPY_FRAME_JPEG (JPEG444) frame at quality q: `total` - 4, the bytes POPPY_SINK_MJPEG writes.
 *   Search.  With qmax the context's quality:
 *         if size(qmax) <= B: the quality is qmax
 *         lo = 0; hi = qmax                  (hi is known not to fit; lo = 0: nothing known to fit)
 *         while hi - lo > 1:  mid = (lo + hi) >> 1;  if size(mid) <= B: lo = mid, else: hi = mid
 *         the quality is max(lo, 1)
 *      At most 1 + ceil(log2(qmax)) qualities are asked about, 8 at qmax = 100.  The search IS the rule, not "the highest quality that fits": size is not monotone
 *      in q on small frames (an 8 x 8 frame of noise has qualities whose file is shorter than the quality below's), the two disagree there, and a rule that needs
 *      all 100 sizes costs 100 measurements where this one costs 8.  On frames of 40 x 24 pixels of noise and more, and on a morph's frames, they coincide.
 *      poppy_jpeg_budget_pick(sizes, qmax, B) is the search alone on a table sizes[1..qmax] (entry 0 is not read): the quality, or POPPY_E_ARG for a null table,
 *      qmax outside 1..100 or B = 0.
 *   Output.  The frame is byte for byte the POPPY_FRAME_JPEG (JPEG444) frame of the same planes at the picked quality: the header with that quality's DQT, the
 *      layout, the capacity, the smallest frame and stride 0 are the format's.  poppy_jpeg_frame_quality(frame) reads the quality back: the largest q in 1..100
 *      whose two tables are the frame's DQT entries, 0 if none is or the frame is not one of this library's JPEG frames (bytes 4, 5 not FF D8, no DQT at the fixed
 *      offset); it serves all six JPEG formats.
 *   No memory between frames.  A frame is a pure function of (planes, qmax, B).
 *   When nothing fits.  If not even quality 1 fits, the frame is the quality-1 frame and exceeds the budget: a frame is always produced, and the caller sees the
 *      overshoot from `total`.
 * poppy_i420_to_jpeg_budget_frame and poppy_i444_to_jpeg_budget_frame are the host statements, poppy_bgr_to_jpeg_budget_frame and
 * poppy_bgr_to_jpeg444_budget_frame the conversion followed by them: the fixed-quality functions' arguments with quality_max and budget in the quality's place, and
 * quality_used (may be null), which receives the picked quality.  They refuse what the fixed-quality functions refuse, and a budget of 0 or above 2^32 - 1 with
 * POPPY_E_ARG.  poppy_hip_i420_to_jpeg_budget_frame and poppy_hip_i444_to_jpeg_budget_frame run the search and the coder on the context's GPU on host planes
 * (upload, the measuring and picking kernels, the two coding kernels, download of `total` bytes): the same bytes and quality; they need no resident pair, disturb
 * none, and neither read nor change the context's own budget and quality.
 * poppy_hip_set_jpeg_budget follows poppy_hip_set_jpeg_quality's contract: POPPY_E_ARG above 2^32 - 1, POPPY_E_STATE while a sequence is open, the context's
 * frames are drained first, and on a refusal the setting stays as it was.  poppy_hip_get_jpeg_budget reads it.  The budget is applied by POPPY_FRAME_JPEG and
 * POPPY_FRAME_JPEG444 only — wherever they apply: poppy_hip_morph, poppy_hip_morph_frames, poppy_hip_render_many, poppy_hip_render_phases,
 * poppy_hip_morph_list and pools, the phase 0 / 1 and t == 0 / 1 copies and the POPPY_E_NOMATCH frames included, under poppy_hip_set_frame_scale and
 * poppy_hip_set_frame_size on the frame at the writer's geometry.  The four formats on built tables (_OPT, _SEQ) have no budget form: a positive budget together
 * with one of them is refused with POPPY_E_UNSUPPORTED by whichever of poppy_hip_set_frame_format and poppy_hip_set_jpeg_budget comes second, and the earlier
 * setting stays.  The other formats ignore the budget as they ignore the quality.  poppy_hip_pool_set_jpeg_budget sets every context of a pool (POPPY_E_STATE
 * with work submitted).  POPPY_SINK_MJPEG takes the frames as they are: every frame is a complete file, and the sink does not read DQT.
 *
 * JPEG sequence budget: POPPY_FRAME_JPEG and POPPY_FRAME_JPEG444 frames whose files TOGETHER have at most B bytes, all coded at ONE quality — "this morph must come
 * out under B bytes as a file", without the pumping of per-frame qualities and without the easy frames leaving their share unused.
 * poppy_hip_set_jpeg_sequence_budget(ctx, B) sets it; 0 (the default) is off and leaves every frame, byte, launch and timing mark as it is without.
 *   Sequence.  Exactly what it is under POPPY_FRAME_JPEG_SEQ: all frames one call hands to its writer; one pair's frames in poppy_hip_morph_list and in the
 *      pools; the t == 0 / 1 copies of poppy_hip_render_phases and the phase 0 / 1 short-circuits count among them, N copies of one frame being its size N times.
 *      The frames wait on the GPU as the planes of their sampling; the writer is first called after the last frame is rendered, and gets the frames in order.
 *   Size.  size_k(q) is the per-frame budget's size: the JFIF file of frame k at quality q, `total` - 4, the bytes POPPY_SINK_MJPEG writes for it.  size(q) is the
 *      sum of size_k(q) over the sequence's frames, in 64 bits.  A container's own bytes are NOT counted — the AVI's index and chunk headers are a constant per
 *      frame, and a caller with a file-size target subtracts them from B itself: the rule is about the frames.
 *   Search.  The per-frame budget's search, word for word, on size(q), with qmax the context's quality: qmax if size(qmax) <= B, otherwise the bisection from
 *      (lo, hi) = (0, qmax), the result max(lo, 1).  The search is the rule, not "the highest quality that fits"; poppy_jpeg_budget_pick on the table of the sums
 *      is its host statement, and B has no 32-bit limit.  At most 1 + ceil(log2(qmax)) qualities are asked about.
 *   Output.  Every frame is byte for byte its POPPY_FRAME_JPEG (JPEG444) frame at the picked quality; the layout, the capacity, the smallest frame and stride 0 are
 *      the format's.  poppy_jpeg_frame_quality reads the quality back from any of the frames.
 *   A sequence of one frame is byte for byte that frame's per-frame-budget frame for the same B.
 *   When nothing fits.  If not even quality 1 fits, the frames are the quality-1 frames, and the caller sees the overshoot from the `total`s.
 * poppy_i420_frames_to_jpeg_seq_budget_frames and poppy_i444_frames_to_jpeg_seq_budget_frames are the host statements, poppy_bgr_frames_to_jpeg_seq_budget_frames
 * and poppy_bgr_frames_to_jpeg444_seq_budget_frames the conversion followed by them: the arguments of poppy_i420_frames_to_jpeg_seq_frames /
 * poppy_bgr_frames_to_jpeg_seq_frames with quality_max and budget in the quality's place; frame k goes to dst + k * poppy_frame_bytes(POPPY_FRAME_JPEG or
 * POPPY_FRAME_JPEG444, width, height); quality_used (may be null) receives the one quality.  Refusals, all from the arguments alone: POPPY_E_ARG for what the
 * _seq_frames functions refuse with it, quality_max outside 1..100 and budget 0; POPPY_E_UNSUPPORTED for JPEG's per-frame limits.  There is no limit on the
 * sequence: a frame's capacity is below 2^32 and the frame count is an int, so the worst case always fits the 64-bit sums.
 * poppy_hip_bgr_frames_to_jpeg_seq_budget_frames and poppy_hip_bgr_frames_to_jpeg444_seq_budget_frames give the same bytes and quality from the context's GPU, on
 * a sequence that lives for the call (upload, raster kernel per frame, the search's steps of one measuring launch over all frames and one pick, the two coding
 * kernels per frame, download of `total` bytes): no resident pair needed, none disturbed, the context's own settings neither read nor changed.
 * poppy_hip_set_jpeg_sequence_budget follows poppy_hip_set_jpeg_budget's contract: POPPY_E_STATE while a sequence is open, the context's frames are drained first,
 * and on a refusal the setting stays as it was; poppy_hip_get_jpeg_sequence_budget reads it.  A context has one of the two budgets: a positive sequence budget
 * together with a positive per-frame budget, or with one of the four formats on built tables (_OPT, _SEQ), is refused with POPPY_E_UNSUPPORTED by whichever of
 * poppy_hip_set_jpeg_sequence_budget, poppy_hip_set_jpeg_budget and poppy_hip_set_frame_format comes second, and the earlier setting stays.  It applies wherever
 * POPPY_FRAME_JPEG_SEQ applies, under poppy_hip_set_frame_scale and poppy_hip_set_frame_size on the frames at the writer's geometry; every other format ignores
 * it, and poppy_hip_morph_sharded and poppy_hip_morph_pairs stay BGR.  poppy_hip_pool_set_jpeg_sequence_budget sets every context of a pool (POPPY_E_STATE with
 * work submitted).  POPPY_SINK_MJPEG takes the frames as they are.
 *
 * POPPY_FRAME_PNG: the frame coded on the GPU as one PNG file, LOSSLESS: the file decodes to exactly the frame's pixels, at 1.5 - 3 times fewer bytes than BGR on
 * photograph-like frames.  Its value is 1024, and POPPY_SINK_PNG is 1024; 1023 and 1025 stay unknown in both enums.  Layout, little-endian:
 *     bytes 0..3     total: the whole frame's length in bytes, these four included (poppy_png_frame_bytes reads it)
 *     bytes 4..      one complete PNG file
 * The writer gets (frame, width, height, stride = 0).  Integer arithmetic throughout; the host statement and the GPU agree byte for byte.
 *   File.  The 8-byte signature; IHDR (width, height, bit depth 8, colour type 2 = RGB, compression 0, filter 0, interlace 0); ONE IDAT holding the whole zlib
 *      stream; IEND.  No ancillary chunks.  Chunk CRCs are the PNG specification's (CRC-32 over type and data).  IDAT's length field is at frame offset 37, the
 *      zlib stream begins at 45, the deflate bits at 47.
 *   Filtered stream.  n = h * (1 + 3 w) bytes: every row is its filter-type byte and 3 w filtered bytes of R, G, B (the frame's BGR swapped; bpp = 3).  All five
 *      filter types of the PNG specification (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) are evaluated for EVERY row from the original pixels; the row above row 0
 *      and the pixel left of column 0 are zeros; Average is floor((a + b) / 2); Paeth takes the specification's tie order a, b, c.  A type's score is the sum over
 *      the row's 3 w filtered bytes v of min(v, 256 - v); the smallest score wins, ties go to the lowest type number.
 *   Segments.  The filtered stream is one linear run, cut into segments of POPPY_PNG_SEGMENT_BYTES = 8192 bytes whatever the rows; the last may be shorter.  The
 *      length is a constant of the FORMAT ("PNG hand-off", says what stands behind its value).
 *   Tables.  POPPY_PNG_TABLES = 8 code-length tables over 257 symbols, literal 0..255 and end-of-block 256; no length or distance symbol is ever emitted: there is
 *      no LZ77 matching.  The tables are constants of the format, committed in poppy_amd/csrc/png_tables.h (poppy_png_table hands them out): table k is an
 *      optimal length-limited (15 bits) prefix code over the weights w(v) = max(1, floor(2^40 * theta_k^m)), m = min(v, 256 - v), theta_k = 1/4, 1/2, 3/4, 7/8,
 *      15/16, 31/32, 63/64, 1, end-of-block weighing 1 (tools/gen_png_tables.py states the construction and its tie rule; the committed header is the
 *      definition).  Codes are deflate's canonical codes from the lengths.
 *   Block header.  Each table has a constant header bit string of H_k bits, in the same file: BFINAL (bit 0), BTYPE = 10, HLIT = 0 (257 codes), HDIST = 0 with one
 *      distance code of length 1, HCLEN, the code-length code's lengths (themselves limited to 7 bits), then the 258 lengths each sent as itself (no run symbols).
 *   Table choice.  Segment s takes the k that minimises H_k + sum of len_k[v] over its bytes + len_k[256]; ties go to the lowest k.
 *   Stream.  78 01; then for every segment in order, NOT byte-aligned, packed from the least significant bit as deflate packs (Huffman codes most significant bit
 *      first, everything else least significant first): the table's header with BFINAL = 1 only in the last segment, the segment's literal codes, end-of-block;
 *      then zero bits to a byte boundary; then the Adler-32 of the filtered stream, big-endian.
 *   Capacity.  poppy_frame_bytes(POPPY_FRAME_PNG, w, h) is an upper bound for any content: table 7 is always a candidate, so a segment of s bytes costs at most
 *      H_7 + L7 * s + len_7[256] bits, L7 <= 9 being table 7's longest literal; summed over the segments and rounded up to bytes, plus 67: `total`, 8 bytes of
 *      signature, 25 of IHDR, 12 of IDAT's framing, 2 of zlib header, 4 of Adler-32 and 12 of IEND.  About 1.13 bytes per byte of BGR.
 *   Limits (POPPY_E_UNSUPPORTED, before any state changes): a capacity of 2^31 bytes or more (IDAT's length field and `total`); poppy_frame_bytes gives 0 for such a size.
 * poppy_bgr_to_png_frame is the host statement (dst: the capacity; POPPY_E_ARG for a null pointer, an empty frame or stride < 3 * width).  poppy_png_table gives
 * table k's 257 lengths and its header bit string (header_bits: POPPY_PNG_HEADER_BYTES bytes, bit i of the string is bit i mod 8 of byte i / 8; either output
 * may be null; POPPY_E_ARG for k outside 0..7).  poppy_hip_bgr_to_png_frame codes a host frame on the context's GPU (upload, the kernels, download of `total`
 * bytes): the same bytes; it needs no resident pair and disturbs none, and places its source as poppy_hip_bgr_downscale does.  The format applies wherever JPEG
 * applies, under poppy_hip_set_frame_scale and poppy_hip_set_frame_size as the host statement at the writer's geometry, and stays BGR wherever JPEG stays BGR.
 *
 * POPPY_FRAME_PNG_RUNS: POPPY_FRAME_PNG with the runs of equal bytes in the filtered stream coded as deflate matches at distance 1: flat, black and smooth
 * regions, which are runs of zeros behind the row filter, cost a few bits per 258 bytes where POPPY_FRAME_PNG pays at least a bit per byte.  Its value is 2048;
 * 2047 and 2049 stay unknown in both enums; there is no sink value of its own: POPPY_SINK_PNG takes both formats.  The format is POPPY_FRAME_PNG word for word —
 * layout and offsets, File, Filtered stream, Segments, 78 01, blocks that are not byte-aligned, BFINAL in the last, Adler-32 over the filtered stream, one IDAT,
 * IEND, Limits — with these changes only:
 *   Tokens.  Within ONE segment, take the maximal runs of equal bytes; a run never extends across a segment cut (so a segment's first byte is always a literal
 *      and blocks stay independent), and a row's filter-type byte is an ordinary byte of the stream that breaks or joins runs like any other.  Of a run of r
 *      bytes the first is a literal.  Let m = r - 1.  If m < POPPY_PNG_RUN_MIN = 8, all m bytes are literals.  Otherwise floor(m / 258) matches of length 258
 *      at distance 1, then for rem = m mod 258: one match of length rem at distance 1 if rem >= 3, rem literals if rem is 1 or 2, nothing if it is 0.  A match
 *      is deflate's length symbol (257..285, RFC 1951 section 3.2.5; length 258 is symbol 285) under the block's table, its extra bits least significant bit
 *      first, then distance symbol 0 (distance 1, no extra bits), which is one 0 bit: the distance table has that one code, of length 1.
 *   Tables.  POPPY_PNG_TABLES = 8 code-length tables over 286 symbols, committed in poppy_amd/csrc/png_runs_tables.h (poppy_png_runs_table hands them out): the
 *      literals and end-of-block weigh what they weigh in POPPY_FRAME_PNG's table k, length symbol 285 weighs max(1, floor(2^40 * theta_k^3)) and each of
 *      257..284 max(1, floor(2^40 * theta_k^6)); the same optimal length-limited (15 bits) construction and tie rule (tools/gen_png_tables.py --runs; the committed
 *      header is the definition).
 *   Block header.  A constant bit string of H_k bits per table, in the same file: BFINAL (bit 0), BTYPE = 10, HLIT = 29 (286 codes), HDIST = 0, HCLEN, the
 *      code-length code's lengths (limited to 7 bits), then the 287 lengths (286 and the distance code's 1) as one sequence in which a length that equals the one
 *      before it and begins r >= 3 equal lengths is sent as symbol 16 with the count min(r, 6); every header fits POPPY_PNG_HEADER_BYTES.
 *   Table choice.  Segment s takes the k that minimises H_k + the bits of all its tokens (codes, extra bits, a bit per match for the distance) + len_k[256]; ties
 *      go to the lowest k.
 *   Capacity.  poppy_frame_bytes(POPPY_FRAME_PNG_RUNS, w, h) is an upper bound for any content: table 7 is always a candidate, a literal costs at most L7r <= 9
 *      bits under it, a match covers at least 3 bytes and costs at most 3 * L7r bits under it (png_runs_tables.h asserts it for every length symbol), so a
 *      segment of s bytes costs at most H_7 + L7r * s + len_7[256] bits; the rest as POPPY_FRAME_PNG's, with this format's H_7 and len_7[256].
 * poppy_bgr_to_png_runs_frame is the host statement (dst: the capacity; the refusals are poppy_bgr_to_png_frame's).  poppy_png_runs_table gives table k's 286
 * lengths and its header bit string as poppy_png_table does.  poppy_png_frame_bytes reads `total` of either format.  poppy_hip_bgr_to_png_runs_frame codes a host
 * frame on the context's GPU as poppy_hip_bgr_to_png_frame does: the same bytes as the host statement.  The format applies wherever POPPY_FRAME_PNG applies and
 * stays BGR wherever that stays BGR.
 *
 * POPPY_FRAME_PNG_OPT: POPPY_FRAME_PNG_RUNS with a ninth candidate per segment, a code built from the segment's OWN symbol counts, in which a symbol that does
 * not occur has no code: a run-free segment does not pay for length symbols it never emits, and a flat one does not pay for literals.  Its value is 16384; 16383
 * and 16385 stay unknown in both enums; there is no sink value of its own: POPPY_SINK_PNG takes the frames and poppy_png_frame_bytes reads `total`.  The format is
 * POPPY_FRAME_PNG_RUNS word for word — layout and offsets, File, Filtered stream, Segments, Tokens (runs never cross a cut, POPPY_PNG_RUN_MIN), 78 01, blocks that
 * are not byte-aligned, BFINAL in the last, Adler-32, one IDAT, IEND, Limits — with these changes only:
 *   Tables.  Per segment, count[s] for s in 0..285 is how often the segment's tokens hold literal or length symbol s, and count[256] = 1, so at least two symbols
 *      have a count.  The own table's lengths are poppy_png_optimal_lengths(count, 286, 15), the rule below; codes are deflate's canonical codes by (length, symbol).
 *      The rule, poppy_jpeg_optimal_table's merges without the reserved entry, for n symbols and a limit of 7 or 15:
 *      1. Every symbol with a count is its own tree.
 *      2. Until there is no c2: c1 is the smallest non-zero count, the largest index among equals; c2 the same among the rest; count[c1] += count[c2],
 *         count[c2] = 0; every symbol of both trees gets one bit longer; c2's tree joins c1's.
 *      3. Count the symbols of each depth.
 *      4. T.81 Annex K.3 from the longest depth down to limit + 1, with `limit` in the place of 16.
 *      5. The symbols with a count, ordered by their depth before step 4 and then by symbol value, take the adjusted lengths in ascending order; every other
 *         symbol gets 0.  A single symbol with a count gets length 1.
 *      A segment has at most 8193 tokens, so depths above 15 do occur (counts 1, 1, 2, 3, 5, 8, ...: depth 16 from a sum of 4179).
 *   Block header.  The eight tables keep their committed headers.  An own header is BFINAL, BTYPE = 10, HLIT = max(257, highest symbol with a length + 1) - 257,
 *      HDIST = 0 with the one distance code of length 1 (even when the block has no match), HCLEN, the code-length code's lengths in RFC 1951's order (16, 17, 18,
 *      0, 8, 7, ...; trailing zeros trimmed, at least 4), then the HLIT + 258 lengths as ONE sequence, lit/len first and then the distance code's 1, cut into
 *      maximal runs of equal values.  A run of r zeros: while r >= 11, symbol 18 with min(r, 138); then symbol 17 with r if r >= 3; else r zeros.  A run of r
 *      equal non-zero lengths: the length once; while the rest is >= 3, symbol 16 with min(rest, 6); what is left as itself.  The code-length code is
 *      poppy_png_optimal_lengths at limit 7 on the counts of the sequence's entries over the 19 symbols, canonical codes again.  An own header is at most
 *      17 + 19 * 3 + 287 * 7 = 2083 bits: no entry costs more than 7 bits per length it covers.
 *   Table choice.  Nine candidates: POPPY_FRAME_PNG_RUNS' tables 0..7 and 8, the own table.  A candidate's cost is its header bits + the tokens' codes + the
 *      matches' extra and distance bits + its end-of-block code; the smallest wins, ties go to the lowest index.
 *   Capacity.  Every block is therefore no longer than POPPY_FRAME_PNG_RUNS' block of the same segment: total(PNG_OPT) <= total(PNG_RUNS) for every frame, and
 *      poppy_frame_bytes(POPPY_FRAME_PNG_OPT, w, h) is POPPY_FRAME_PNG_RUNS' capacity.
 * poppy_bgr_to_png_opt_frame is the host statement (dst: the capacity; the refusals are poppy_bgr_to_png_frame's).  poppy_png_optimal_lengths is the length rule
 * alone, host only, integers only: `lengths` receives n_symbols bytes; POPPY_E_ARG for a null pointer, n_symbols outside 1..286, a limit other than 7 or 15,
 * counts that are all zero, a sum of 2^32 or more, and more symbols with a count than 2^limit (no code of that length holds them).
 * poppy_hip_bgr_to_png_opt_frame codes a host frame on the context's GPU as poppy_hip_bgr_to_png_runs_frame does, and poppy_hip_png_optimal_lengths runs the
 * device's length build alone on given counts, as poppy_hip_jpeg_optimal_table does: the same bytes as the host statements, with their refusals.  The format
 * applies wherever POPPY_FRAME_PNG_RUNS applies and stays BGR wherever that stays BGR.
 *
 * POPPY_FRAME_PNG_SEQ: POPPY_FRAME_PNG_OPT with ONE ninth table for all the frames a call hands to its writer, built from the summed symbol counts of the whole
 * sequence: the build runs once per sequence, not once per segment, and its 900-bit header is paid only by the segments that choose it.  Its value is 131072;
 * 131071 and 131073 stay unknown in both enums; there is no sink value of its own: POPPY_SINK_PNG takes the frames and poppy_png_frame_bytes reads `total`.  The
 * format is POPPY_FRAME_PNG_OPT word for word — layout and offsets, File, Filtered stream, Segments of POPPY_PNG_SEGMENT_BYTES, Tokens with POPPY_PNG_RUN_MIN,
 * 78 01, blocks that are not byte-aligned, BFINAL in a frame's last block, Adler-32, one IDAT, IEND — with these changes only:
 *   Counts.  For s in 0..285, count[s] is how often the tokens of all segments of all frames of the sequence hold literal or length symbol s; count[256] is the
 *      number of segments of the sequence, one end-of-block per block.  A frame that stands in the sequence N times counts N times.
 *   Table.  poppy_png_optimal_lengths(count, 286, 15), the unchanged rule, once per sequence; codes are the canonical codes by (length, symbol).  A symbol that
 *      some segment never emits still has a code, because another segment gave it a count; a symbol no segment emits has none.
 *   Block header.  POPPY_FRAME_PNG_OPT's own-header rule applied to the sequence's lengths: HLIT from the highest symbol with a length, HDIST = 0, the run-coded
 *      length sequence on its own 7-bit code-length code.  It is one bit string per sequence, of at most 2083 bits; BFINAL, bit 0, is set in a frame's last
 *      block only.
 *   Table choice.  Nine candidates per segment: POPPY_FRAME_PNG_RUNS' tables 0..7, and 8, the sequence's table.  A candidate's cost is its header bits + the
 *      tokens' codes + the matches' extra and distance bits + its end-of-block code; the smallest wins, ties go to the lowest index: table 8 wins only outright.
 *   Consequences.  Every block is no longer than POPPY_FRAME_PNG_RUNS' block of the same segment: total(PNG_SEQ) <= total(PNG_RUNS) for every frame of every
 *      sequence, and poppy_frame_bytes(POPPY_FRAME_PNG_SEQ, w, h) is POPPY_FRAME_PNG_RUNS' capacity.  A sequence of one frame of one segment is byte for byte
 *      that frame's POPPY_FRAME_PNG_OPT frame.  Every frame decodes to exactly its pixels.  The order of the frames changes no table.
 *   Limits, checked on the arguments alone before any state changes, refused with POPPY_E_UNSUPPORTED.  Per frame: POPPY_FRAME_PNG_RUNS'.  Per sequence: with
 *      n = h (1 + 3 w) and S = ceil(n / 8192), n_frames * (n + S) <= POPPY_PNG_SEQ_MAX_SYMBOLS = 2^32 - 1.  A segment of s bytes has at most s tokens and one
 *      end-of-block, so the sum of the counts stays under the length rule's own refusal and the device adds in 32 bits.  That allows 690 frames at 1080p.
 *   Sequence.  Exactly what it is under POPPY_FRAME_JPEG_SEQ: all the frames one call hands to its writer; in poppy_hip_morph_list and in the pool one pair's
 *      frames.  The t = 0 / t = 1 copies of poppy_hip_render_phases, the phase-0 / phase-1 short-circuits and the POPPY_E_NOMATCH linear-blend frames count as
 *      POPPY_FRAME_JPEG_SEQ counts them.  The frames wait on the device as filtered streams; the writer is first called after the last frame is rendered and gets
 *      the frames in order, as (frame, width, height, stride = 0).
 * poppy_bgr_frames_to_png_seq_frames is the host statement: poppy_bgr_frames_to_jpeg_seq_frames' arguments without the quality, frame k into dst +
 * k * poppy_frame_bytes(POPPY_FRAME_PNG_SEQ, width, height); POPPY_E_ARG for a null pointer, n_frames < 1, an empty frame, a stride shorter than a row or a
 * frame_stride shorter than a frame, POPPY_E_UNSUPPORTED for the limits; both before a byte is read.  poppy_png_seq_table gives the table and its header bit
 * string (BFINAL 0; header_bits: POPPY_PNG_SEQ_HEADER_BYTES bytes, bit i of the string is bit i mod 8 of byte i / 8; either output may be null) from given counts:
 * poppy_png_optimal_lengths' refusals, and POPPY_E_ARG too where count[256] is 0.  poppy_hip_bgr_frames_to_png_seq_frames does the same on the context's GPU, in a
 * sequence that lives for the call and disturbs neither a resident pair nor the context's own sequence, and poppy_hip_png_seq_table runs the device's table build
 * alone on given counts: the same bytes as the host statements, with their refusals.  The format applies wherever POPPY_FRAME_PNG_RUNS applies and stays BGR
 * wherever that stays BGR.  */
#define POPPY_PAL8_MAX_PIXELS (1 << 24)
#define POPPY_PAL8_SEQ_MAX_PIXELS (1ull << 32)
#define POPPY_GIF_SEGMENT_PIXELS 2048
#define POPPY_GIF_SEGMENT_BYTES ((9 + 12 * (POPPY_GIF_SEGMENT_PIXELS + 2) + 63 + 7) / 8)
#ifndef POPPY_JPEG_RESTART_MCUS      /* (a build with another value codes ANOTHER format: only for measuring what the choice costs) */
#define POPPY_JPEG_RESTART_MCUS 8
#endif
#define POPPY_JPEG_SEGMENT_BYTES (2 * ((6 * 1660 * POPPY_JPEG_RESTART_MCUS + 7) / 8) + 2)
#define POPPY_JPEG_OPT_SEGMENT_BYTES (2 * ((6 * 1661 * POPPY_JPEG_RESTART_MCUS + 7) / 8) + 2)
#define POPPY_JPEG_SEQ_MAX_SYMBOLS 0xfffffffeull      /* (n_frames * blocks of a frame * 64 at the most: POPPY_FRAME_JPEG_SEQ, Limits) */
#define POPPY_JPEG444_RESTART_MCUS 16      /* (3 * 16 blocks = 6 * POPPY_JPEG_RESTART_MCUS: poppy_amd/csrc/jpeg_tables.h asserts it) */
#define POPPY_JPEG_QUALITY_DEFAULT 90
#define POPPY_PNG_SEGMENT_BYTES 8192
#define POPPY_PNG_TABLES 8
#define POPPY_PNG_HEADER_BYTES 236      /* (any header of the form fits: 17 + 19 * 3 + 258 * 7 bits) */
#define POPPY_PNG_RUN_MIN 8
#define POPPY_PNG_SEQ_MAX_SYMBOLS 0xffffffffull      /* (n_frames * (stream bytes + segments of a frame) at the most: POPPY_FRAME_PNG_SEQ, Limits) */
#define POPPY_PNG_SEQ_HEADER_BYTES 261      /* (the sequence's header fits: 17 + 19 * 3 + 287 * 7 = 2083 bits) */
enum { POPPY_FRAME_BGR = 0, POPPY_FRAME_I420 = 1, POPPY_FRAME_PAL8 = 8, POPPY_FRAME_PAL8_SEQ = 16, POPPY_FRAME_GIF = 64, POPPY_FRAME_GIF_SEQ = 128, POPPY_FRAME_JPEG = 256,
       POPPY_FRAME_JPEG444 = 512, POPPY_FRAME_PNG = 1024, POPPY_FRAME_PNG_RUNS = 2048, POPPY_FRAME_JPEG_OPT = 4096,
       POPPY_FRAME_JPEG444_OPT = 8192, POPPY_FRAME_PNG_OPT = 16384, POPPY_FRAME_JPEG_SEQ = 32768, POPPY_FRAME_JPEG444_SEQ = 65536,
       POPPY_FRAME_PNG_SEQ = 131072 };
int poppy_hip_set_frame_format(poppy_hip_ctx* ctx, int format);
size_t poppy_frame_bytes(int format, int width, int height);
int poppy_bgr_to_i420(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst);
int poppy_bgr_to_pal8(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst);
int poppy_bgr_frames_to_pal8(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, uint8_t* dst);
size_t poppy_gif_frame_bytes(const uint8_t* frame);
int poppy_pal8_to_gif_frame(const uint8_t* pal8, int width, int height, uint8_t* dst);
int poppy_bgr_to_gif_frame(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst);
int poppy_hip_pal8_to_gif_frame(poppy_hip_ctx* ctx, const uint8_t* pal8, int width, int height, uint8_t* dst);
int poppy_bgr_frames_to_gif_frames(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, uint8_t* dst);
int poppy_hip_bgr_frames_to_gif_frames(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, uint8_t* dst);
size_t poppy_jpeg_frame_bytes(const uint8_t* frame);
int poppy_i420_to_jpeg_frame(const uint8_t* i420, int width, int height, int quality, uint8_t* dst);
int poppy_bgr_to_jpeg_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality, uint8_t* dst);
int poppy_hip_i420_to_jpeg_frame(poppy_hip_ctx* ctx, const uint8_t* i420, int width, int height, int quality, uint8_t* dst);
int poppy_hip_set_jpeg_quality(poppy_hip_ctx* ctx, int quality);
int poppy_bgr_to_i444(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst);
int poppy_hip_bgr_to_i444(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst);
int poppy_i444_to_jpeg_frame(const uint8_t* i444, int width, int height, int quality, uint8_t* dst);
int poppy_bgr_to_jpeg444_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality, uint8_t* dst);
int poppy_hip_i444_to_jpeg_frame(poppy_hip_ctx* ctx, const uint8_t* i444, int width, int height, int quality, uint8_t* dst);
int poppy_jpeg_budget_pick(const uint32_t* sizes, int quality_max, size_t budget);
int poppy_jpeg_frame_quality(const uint8_t* frame);
int poppy_i420_to_jpeg_budget_frame(const uint8_t* i420, int width, int height, int quality_max, size_t budget, uint8_t* dst, int* quality_used);
int poppy_i444_to_jpeg_budget_frame(const uint8_t* i444, int width, int height, int quality_max, size_t budget, uint8_t* dst, int* quality_used);
int poppy_bgr_to_jpeg_budget_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality_max, size_t budget, uint8_t* dst, int* quality_used);
int poppy_bgr_to_jpeg444_budget_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality_max, size_t budget, uint8_t* dst, int* quality_used);
int poppy_hip_i420_to_jpeg_budget_frame(poppy_hip_ctx* ctx, const uint8_t* i420, int width, int height, int quality_max, size_t budget, uint8_t* dst, int* quality_used);
int poppy_hip_i444_to_jpeg_budget_frame(poppy_hip_ctx* ctx, const uint8_t* i444, int width, int height, int quality_max, size_t budget, uint8_t* dst, int* quality_used);
int poppy_hip_set_jpeg_budget(poppy_hip_ctx* ctx, size_t max_frame_bytes);
int poppy_hip_get_jpeg_budget(poppy_hip_ctx* ctx, size_t* max_frame_bytes);
/* JPEG sequence budget (above): the host statements, the same from the context's GPU, and the setting; 0 (the default): off */
int poppy_i420_frames_to_jpeg_seq_budget_frames(const uint8_t* i420, size_t frame_stride, int n_frames, int width, int height, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used);
int poppy_i444_frames_to_jpeg_seq_budget_frames(const uint8_t* i444, size_t frame_stride, int n_frames, int width, int height, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used);
int poppy_bgr_frames_to_jpeg_seq_budget_frames(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used);
int poppy_bgr_frames_to_jpeg444_seq_budget_frames(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used);
int poppy_hip_bgr_frames_to_jpeg_seq_budget_frames(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used);
int poppy_hip_bgr_frames_to_jpeg444_seq_budget_frames(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality_max, uint64_t budget, uint8_t* dst, int* quality_used);
int poppy_hip_set_jpeg_sequence_budget(poppy_hip_ctx* ctx, uint64_t max_sequence_bytes);
int poppy_hip_get_jpeg_sequence_budget(poppy_hip_ctx* ctx, uint64_t* max_sequence_bytes);
int poppy_jpeg_optimal_table(const uint32_t counts[256], uint8_t bits[16], uint8_t vals[256], int* n_vals);
int poppy_i420_to_jpeg_opt_frame(const uint8_t* i420, int width, int height, int quality, uint8_t* dst);
int poppy_i444_to_jpeg_opt_frame(const uint8_t* i444, int width, int height, int quality, uint8_t* dst);
int poppy_bgr_to_jpeg_opt_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality, uint8_t* dst);
int poppy_bgr_to_jpeg444_opt_frame(const uint8_t* bgr, size_t stride, int width, int height, int quality, uint8_t* dst);
int poppy_hip_i420_to_jpeg_opt_frame(poppy_hip_ctx* ctx, const uint8_t* i420, int width, int height, int quality, uint8_t* dst);
int poppy_hip_i444_to_jpeg_opt_frame(poppy_hip_ctx* ctx, const uint8_t* i444, int width, int height, int quality, uint8_t* dst);
int poppy_hip_jpeg_optimal_table(poppy_hip_ctx* ctx, const uint32_t counts[256], uint8_t bits[16], uint8_t vals[256], int* n_vals);
int poppy_i420_frames_to_jpeg_seq_frames(const uint8_t* i420, size_t frame_stride, int n_frames, int width, int height, int quality, uint8_t* dst);
int poppy_i444_frames_to_jpeg_seq_frames(const uint8_t* i444, size_t frame_stride, int n_frames, int width, int height, int quality, uint8_t* dst);
int poppy_bgr_frames_to_jpeg_seq_frames(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality, uint8_t* dst);
int poppy_bgr_frames_to_jpeg444_seq_frames(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality, uint8_t* dst);
int poppy_hip_bgr_frames_to_jpeg_seq_frames(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality, uint8_t* dst);
int poppy_hip_bgr_frames_to_jpeg444_seq_frames(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, int quality, uint8_t* dst);
size_t poppy_png_frame_bytes(const uint8_t* frame);
int poppy_png_table(int k, uint8_t lengths[257], uint8_t* header_bits, int* n_header_bits);
int poppy_bgr_to_png_frame(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst);
int poppy_hip_bgr_to_png_frame(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst);
int poppy_png_runs_table(int k, uint8_t lengths[286], uint8_t* header_bits, int* n_header_bits);
int poppy_bgr_to_png_runs_frame(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst);
int poppy_hip_bgr_to_png_runs_frame(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst);
int poppy_png_optimal_lengths(const uint32_t* counts, int n_symbols, int limit, uint8_t* lengths);
int poppy_bgr_to_png_opt_frame(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst);
int poppy_hip_bgr_to_png_opt_frame(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst);
int poppy_hip_png_optimal_lengths(poppy_hip_ctx* ctx, const uint32_t* counts, int n_symbols, int limit, uint8_t* lengths);
int poppy_png_seq_table(const uint32_t counts[286], uint8_t lengths[286], uint8_t* header_bits, int* n_header_bits);
int poppy_bgr_frames_to_png_seq_frames(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, uint8_t* dst);
int poppy_hip_bgr_frames_to_png_seq_frames(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, uint8_t* dst);
int poppy_hip_png_seq_table(poppy_hip_ctx* ctx, const uint32_t counts[286], uint8_t lengths[286], uint8_t* header_bits, int* n_header_bits);
/* Scaled hand-off: frames rendered at the pair's resolution and handed to the writer scaled down by a whole factor, on the GPU, in front of the format
 * conversion.  The pair's resolution decides the keypoints, the mesh and the morph; the scale only decides what crosses the link and what the writer gets.
 *   The rule.  A factor s is a whole number from 1 to POPPY_FRAME_SCALE_MAX = 8; 1, the default, is the identity.  A width x height BGR frame becomes
 *      ow x oh, ow = (width + s - 1) / s, oh = (height + s - 1) / s (poppy_frame_scaled_size).  Output pixel (x, y) covers source columns
 *      [s x, min(s x + s, width)) and rows [s y, min(s y + s, height)), n = 1 .. 64 pixels: blocks are clipped at the right and bottom edges, as I420's chroma
 *      blocks are, and no pixel is dropped.  Per channel out = (sum + n / 2) / n in integer arithmetic; there is no gamma handling.
 *   poppy_bgr_downscale is the host statement (dst: oh rows of 3 * ow bytes, dst_stride >= 3 * ow apart).  POPPY_E_ARG, before anything is read or written,
 *      for a null pointer, an empty frame, a factor outside 1..8, stride < 3 * width or dst_stride < 3 * ow.  poppy_hip_bgr_downscale does the same on the
 *      context's GPU (upload, the kernel, download): the same bytes.  It needs no resident pair and disturbs none.  The device copy of the source is tight and
 *      begins (stride - 3 * width) mod 16 bytes behind a 256-byte boundary, so that a caller (a test) reaches every alignment the kernel's launcher tells apart.
 *   A writer's frame under scale s and format F is F's host statement at the scaled geometry, applied to poppy_bgr_downscale of the BGR frame that a
 *      context with s = 1 hands out: poppy_bgr_to_i420, poppy_bgr_to_pal8, poppy_bgr_frames_to_pal8, poppy_bgr_to_gif_frame, poppy_bgr_frames_to_gif_frames.
 *      Under the sequence formats the palette is taken over the SCALED frames.  The writer is told ow, oh and the format's stride for ow (3 * ow, ow or 0);
 *      a caller opens its sink with poppy_frame_scaled_size.
 *   Limits are the format's, checked on the scaled geometry and the scaled sequence before any state changes (2^24 pixels per frame, 65535 per side, fewer than
 *      2^32 per sequence): a pair that a format refuses at s = 1 can be admissible at s = 2.
 *   Where it applies: exactly where the frame format applies — every frame handed to a writer by poppy_hip_morph, poppy_hip_morph_frames,
 *      poppy_hip_render_many, poppy_hip_render_phases, poppy_hip_morph_list and the calls of a pool (poppy_hip_pool_set_frame_scale), the phase 0 / 1 and
 *      t == 0 / 1 copies and the POPPY_E_NOMATCH blend frames included.  Host images among these are scaled by the host statement.
 *   Where it does not: everything that stays BGR under a format stays full size — poppy_hip_render / poppy_hip_dissolve into an explicit dst,
 *      poppy_hip_frame_device, poppy_hip_debug_fetch, frames kept on the device (write == NULL), poppy_hip_morph_sharded, poppy_hip_morph_pairs and
 *      include/poppy_hip_shim.hpp.  The chain is untouched: corrected1 <- frame is the full-size frame, so the BGR frames of a chained sequence under s > 1
 *      are the scaled frames of the same sequence under s = 1.
 * poppy_hip_set_frame_scale drains the context's frames, as poppy_hip_set_frame_format does; POPPY_E_ARG outside 1..8, POPPY_E_STATE while a sequence is
 * open, POPPY_E_UNSUPPORTED (nothing changed) when the resident pair's scaled frame is refused by the context's format.  It takes effect with or without a
 * resident pair, before or after the format is set.  A factor above 1 returns POPPY_E_STATE while a size is set (poppy_hip_set_frame_size). */
#define POPPY_FRAME_SCALE_MAX 8
int poppy_hip_set_frame_scale(poppy_hip_ctx* ctx, int factor);
int poppy_frame_scaled_size(int width, int height, int factor, int* ow, int* oh);
int poppy_bgr_downscale(const uint8_t* bgr, size_t stride, int width, int height, int factor, uint8_t* dst, size_t dst_stride);
int poppy_hip_bgr_downscale(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, int width, int height, int factor, uint8_t* dst, size_t dst_stride);
/* Resized hand-off: the scaled hand-off with a free size instead of a whole factor — frames rendered at the pair's resolution and handed to the writer as
 * ow x oh frames, resampled on the GPU in front of the format conversion.  A context has a scale above 1 or a size, never both.
 *   The rule: exact area resampling in integer arithmetic.  A width x height BGR frame becomes ow x oh, where 1 <= ow <= width, 1 <= oh <= height,
 *      width <= POPPY_FRAME_SCALE_MAX * ow and height <= POPPY_FRAME_SCALE_MAX * oh: downscale only, by at most 8 per axis; the aspect ratio need not be kept.
 *      Columns are measured in units of 1 / ow of a source pixel: output column x covers [x * width, (x + 1) * width), source column i covers
 *      [i * ow, (i + 1) * ow), and wx(x, i) is the length of their overlap, a whole number 0..ow.  It is non-zero for i from (x * width) / ow to
 *      ((x + 1) * width - 1) / ow; over i it sums to width, over x to ow.  wy(y, r) is the same with height and oh.  Per channel
 *         out(x, y) = (sum over r, i of wy(y, r) * wx(x, i) * src(i, r) + (width * height) / 2) / (width * height)
 *      with integer divisions and the numerator formed in 64 bits; there is no gamma handling.  The numerator is at most 255.5 * width * height, which fits
 *      an unsigned 32-bit word exactly when width * height <= 2^24: the device forms 32-bit sums up to that size and 64-bit sums above it.
 *   Properties.  Identity: ow = width and oh = height returns the frame.  A constant frame stays constant.  Where width = s * ow and height = s * oh the
 *      bytes are exactly those of the whole-factor rule at factor s (every weight is ow resp. oh; DESIGN.md section 4 has the derivation).  Where the
 *      whole-factor rule clips its edge blocks (width % s != 0 or height % s != 0) the two rules differ by design: this one stretches every output pixel
 *      over the same share of the frame, that one clips.
 *   poppy_bgr_resize_area is the host statement (dst: oh rows of 3 * ow bytes, dst_stride >= 3 * ow apart).  POPPY_E_ARG, before anything is read or
 *      written, for a null pointer, an empty frame, an inadmissible size, stride < 3 * width or dst_stride < 3 * ow.  poppy_hip_bgr_resize_area does the
 *      same on the context's GPU (upload, the kernel, download): the same bytes.  It needs no resident pair and disturbs none.  The device copy of the source
 *      is tight and begins (stride - 3 * width) mod 16 bytes behind a 256-byte boundary, so that a caller (a test) reaches every alignment of the source.
 *   poppy_frame_fit_size gives the largest size inside a max_width x max_height box that keeps the aspect ratio: (width, height) itself when the frame fits;
 *      else, when width * max_height >= height * max_width, ow = max_width and oh = max(1, (height * max_width + width / 2) / width), otherwise oh = max_height
 *      and ow = max(1, (width * max_height + height / 2) / height), all products in 64 bits.  POPPY_E_ARG for non-positive arguments or null pointers (the
 *      outputs untouched), POPPY_E_UNSUPPORTED when the result would need more than a factor of 8 on an axis.
 *   A writer's frame under size (ow, oh) and format F is F's host statement at ow x oh, applied to poppy_bgr_resize_area of the BGR frame that a plain
 *      context hands out.  Under the sequence formats the palette is taken over the RESIZED frames.  The writer is told ow, oh and the format's stride for ow.
 *   Limits are the format's, checked on ow x oh and the resized sequence before any state changes.
 *   Where it applies: exactly where the frame format applies — every frame handed to a writer by poppy_hip_morph, poppy_hip_morph_frames,
 *      poppy_hip_render_many, poppy_hip_render_phases, poppy_hip_morph_list and the calls of a pool (poppy_hip_pool_set_frame_size), the phase 0 / 1 and
 *      t == 0 / 1 copies and the POPPY_E_NOMATCH blend frames included.  Host images among these are resized by the host statement.
 *   Where it does not: everything that stays BGR under a format stays full size — poppy_hip_render / poppy_hip_dissolve into an explicit dst,
 *      poppy_hip_frame_device, poppy_hip_debug_fetch, frames kept on the device (write == NULL), poppy_hip_morph_sharded, poppy_hip_morph_pairs and
 *      include/poppy_hip_shim.hpp.  The chain is untouched: corrected1 <- frame is the full-size frame.
 * poppy_hip_set_frame_size: (0, 0), the default, switches the size off.  It drains the context's frames, as poppy_hip_set_frame_scale does.  POPPY_E_ARG for
 * a negative value or when exactly one of the two is 0; POPPY_E_STATE while a sequence is open or while the context's scale is above 1 (symmetrically,
 * poppy_hip_set_frame_scale with a factor above 1 returns POPPY_E_STATE while a size is set; each is switched off to get to the other);
 * POPPY_E_UNSUPPORTED (nothing changed) when the resident pair's geometry does not admit the size or the context's format refuses ow x oh.  It takes effect
 * with or without a resident pair, before or after the format is set.  A pair whose geometry does not admit the set size is refused with
 * POPPY_E_UNSUPPORTED by the call that brings it, before any state changes, as a pair that the format refuses is; a host image that is handed to a writer
 * without a pair (the phase 0 / 1 copies) is refused by that call. */
int poppy_hip_set_frame_size(poppy_hip_ctx* ctx, int ow, int oh);
int poppy_frame_fit_size(int width, int height, int max_width, int max_height, int* ow, int* oh);
int poppy_bgr_resize_area(const uint8_t* bgr, size_t stride, int width, int height, int ow, int oh, uint8_t* dst, size_t dst_stride);
int poppy_hip_bgr_resize_area(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, int width, int height, int ow, int oh, uint8_t* dst, size_t dst_stride);
/* which width of arithmetic the device takes for these sizes: 2 for 32-bit sums and 32-bit indices (width * height <= 2^24, both sides <= 32768), 1 for 32-bit
 * sums and 64-bit indices (width * height <= 2^24, a longer side), 0 for 64-bit sums and indices (above 2^24 pixels); POPPY_E_ARG for an inadmissible size.
 * The sizes alone decide: every alignment of the source is taken. */
int poppy_hip_bgr_resize_area_form(int width, int height, int ow, int oh);
/* phase == 0 / phase == 1 follow the reference's short-circuit (src/poppy.hpp:54-70): number_of_frames copies of image 1 /
 * image 2 as they were handed to the pair set-up (with auto-align: the UNALIGNED image 2), no frame is rendered.            */

/* The whole of poppy::morph(img1, img2, corrected1, corrected2, phase, distance, output) (src/poppy.hpp:46-248) in one call,
 * in the reference's order: phase == 0 / 1 short-circuits (:54-70, before any feature work) -> pair set-up from the raw
 * images (poppy_hip_pair_begin) -> the printed morph distance (:142-159) -> frame loop with the reference's scheduler
 * (:177-235; one frame when 0 < phase < 1).  distance != 0 reproduces --distance: the value is computed, no frame is
 * written and the call returns POPPY_OK (the reference prints it and calls exit(0), :159-163; the shim does that).
 * *morph_distance (may be NULL) receives the printed value whenever the set-up ran.
 * No point pairs: poppy::morph means to write number_of_frames frames of img2*phase + img1*(1-phase) (:125-134) — with the
 * phase ARGUMENT, i.e. -1 in the default mode — but the reference never gets there: with empty point lists Matcher::find ->
 * morph_distance -> cv::convexHull throws first (tried with the golden generator).  This call writes the intended
 * fallback frames and returns POPPY_E_NOMATCH so that a caller can tell; corrected2 comes from poppy_hip_pair_corrected2. */
int poppy_hip_morph(poppy_hip_ctx* ctx, const uint8_t* bgr1, size_t stride1, const uint8_t* bgr2, size_t stride2,
                    int width, int height, double phase, int distance, poppy_write_cb write, void* user,
                    double* morph_distance);
/* The value poppy::morph prints as "morph distance" for the resident pair (src/poppy.hpp:142-159: clip_points, make_uniq,
 * truncate to the shorter list, morph_distance) — what --distance reports.  Host arithmetic, computed on demand.          */
int poppy_hip_pair_distance(poppy_hip_ctx* ctx, double* morph_distance);
/* the same value from explicit point lists (host only, no ctx): points as Matcher::prepare leaves them */
int poppy_printed_morph_distance(const float* points1, const float* points2, int n_points, int width, int height, double* morph_distance);

/* ---- once-per-pair stage (outer boundary: poppy::morph, src/poppy.hpp:46-157) -------------------
 * ORB::create(nfeatures)->detect(gray, keypoints)  (src/extractor.cpp:45,77-78).  gray is an 8-bit single
 * channel host image.  kps7 receives max_kps x 7 floats per keypoint in cv::KeyPoint field order
 * (x, y, size, angle, response, octave, class_id); the ORDER equals the reference's.  retainBest keeps every tie with the
 * n-th response, so the count has no bound in nfeatures: *n_kps is written also when it exceeds max_kps (POPPY_E_ARG, nothing
 * copied), and a second call with that size succeeds.                                                   */
int poppy_hip_orb_detect(poppy_hip_ctx* ctx, const uint8_t* gray, size_t stride, int width, int height,
                         int nfeatures, float* kps7, int max_kps, int* n_kps);

/* North-star kernels WITHOUT a call site in Poppy (it never computes descriptors); pinned against
 * OpenCV directly:  ORB::compute (WTA_K 2, 32 bytes/keypoint; OCV/features2d/src/orb.cpp:219-285,1148-1216) and
 * BFMatcher(NORM_HAMMING).match (OCV/features2d/src/matchers.cpp:757, OCV/core/src/batch_distance.cpp:199-262;
 * rows of out3 = queryIdx, trainIdx, distance; lowest train index wins ties).
 * orb_describe accepts a keypoint (kps7 row: x, y, size, angle, response, octave, class id) whose octave is 0..7 and whose
 * level position cvRound(pt / scale(octave)) lies in [-9, level width + 9) x [-9, level height + 9): the 31 x 31 steered
 * patch around it then stays inside the level's 32-pixel border.  Any other keypoint makes the whole call POPPY_E_ARG.
 * A patch near the border reads that border: the reflect-101 ring around the level, which the reference's in-place
 * GaussianBlur of the level leaves unblurred, and so does this.  The reference's own ORB::compute never gets that far: it
 * drops every keypoint closer than 31 px to the border first (runByImageBorder); callers that want its output keep to
 * keypoints that test would keep, as the detector's are.                                                     */
int poppy_hip_orb_describe(poppy_hip_ctx* ctx, const uint8_t* gray, size_t stride, int width, int height,
                           const float* kps7, int n_kps, uint8_t* descriptors32);
int poppy_hip_hamming_match(poppy_hip_ctx* ctx, const uint8_t* query32, int n_query, const uint8_t* train32, int n_train,
                            int* out3, int* n_matches);

/* Descriptor matching as the reference sketched it (src/experiments.hpp:14-144, dead code there):
 *   hamming_knn2   : BFMatcher(NORM_HAMMING).knnMatch(k = 2) — rows of out4 = trainIdx0, distance0, trainIdx1, distance1,
 *                    ordered by (distance, train index) (OCV/core/src/batch_distance.cpp:225-248), -1 where there is none;
 *   ratio_symmetry : ratioTest (a query survives with two neighbours and distance0 / distance1 <= ratio) on both
 *                    directions, then symmetryTest; rows of out3 = queryIdx, trainIdx, distance.  Host only.
 * ransacTest (findFundamentalMat) of the same sketch: poppy_ransac_fundamental below.                            */
int poppy_hip_hamming_knn2(poppy_hip_ctx* ctx, const uint8_t* query32, int n_query, const uint8_t* train32, int n_train, int* out4);
int poppy_ratio_symmetry(const int* knn12, int n1, const int* knn21, int n2, float ratio, int* out3, int* n_out);

/* The sketch's third filter, ransacTest: the pairs that agree with a fundamental matrix found by RANSAC.  Not OpenCV's findFundamentalMat (its sampler, its
 * 7-point solver and its adaptive iteration count are not restated): the filter is DEFINED by the host statement poppy_ransac_fundamental, and
 * poppy_hip_ransac_fundamental, which scores the hypotheses on the GPU, returns the same bytes.
 *   The hypothesis count is fixed, so the result does not depend on scheduling: with an inlier share of 0.5 a sample of 8 is all inliers with probability
 *   0.5^8 = 1 / 256, and 2048 samples hold at least one such sample with probability 1 - (1 - 0.5^8)^2048 = 1 - e^(2048 ln(255 / 256)) = 1 - e^-8.016 = 0.9997.
 *   All arithmetic is double: + - * / sqrt and comparisons, every sum in a stated order, no fused products, no libm.
 *   Input: n_points pairs (x1, y1) <-> (x2, y2) of floats, 8 <= n_points <= 65536, widened to double; distance d >= 0 in pixels (the sketch: 3.0).
 *   Normalisation, per image, over all points: centroid m (sums in index order, / n), r = the mean of sqrt(dx^2 + dy^2) to it (in index order), s = sqrt(2) / r,
 *     T = [[s, 0, -(s mx)], [0, s, -(s my)], [0, 0, 1]], x^ = s x + T[0][2], y^ = s y + T[1][2].  r = 0 in either image: no model.
 *   Samples: hypothesis h (0 .. 2047) draws 8 distinct indices; draw k (0 .. 7) is r = mix32(0x9E3779B9 (8 h + k + 1)) mod (n - k) in 32-bit wrap-around
 *     arithmetic, mapped onto the indices not yet drawn: for each earlier draw in ascending order of value, r += (r >= value).
 *     mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *   Model: row i of the 8 x 9 system, from draw i, is (x2^ x1^, x2^ y1^, x2^, y2^ x1^, y2^ y1^, y2^, x1^, y1^, 1).  Its null vector by Gaussian elimination with
 *     complete pivoting: at step k (0 .. 7) the pivot is the largest |A[i][j]| over rows i = k .. 7 and columns j = k .. 8 of the matrix as it stands, scanned row by
 *     row, ties to the lowest row and then the lowest column; rows k and i swap, columns k and j swap (the unknowns with them); then for i = k + 1 .. 7:
 *     f = A[i][k] / A[k][k] and for j = k + 1 .. 8: A[i][j] = A[i][j] - f A[k][j].  A first pivot of 0, or any pivot below 1e-10 of the first: the hypothesis is
 *     INVALID.  The free unknown z[8] = 1; for i = 7 .. 0: s = 0, for j = i + 1 .. 8: s = s + A[i][j] z[j]; z[i] = (-s) / A[i][i]; the column swaps are undone: F^
 *     (3 x 3, row-major).  No rank-2 step.  F_h = T2^T (F^ T1): G = F^ T1 first, then T2^T G, every entry (a0 b0 + a1 b1) + a2 b2 with all three products.
 *   Score: a = (F[0][0] x1 + F[0][1] y1) + F[0][2], b and c likewise from rows 1 and 2; e = (a x2 + b y2) + c; a' = (F[0][0] x2 + F[1][0] y2) + F[2][0],
 *     b' = (F[0][1] x2 + F[1][1] y2) + F[2][1], on the points as given (widened).  Pair i is an inlier of h iff e e <= (d d) (a a + b b) and
 *     e e <= (d d) (a' a' + b' b').  counts[h] = the number of inliers, -1 for an invalid hypothesis.
 *   Choice: the largest count, ties to the lowest h.  No valid hypothesis, or a best count below 8: no model.
 *   Result: inliers[i] = 1 / 0, the best hypothesis's inliers in input order; *n_inliers their number; *best = h.  f3x3 (row-major, x2^T F x1 = 0) is a normalised
 *     8-point fit over those inliers (host only, also in the GPU form): the normalisation recomputed from them, A^T A (9 x 9) through cyclic Jacobi and the vector of
 *     its smallest eigenvalue, rank 2 by a 3 x 3 one-sided Jacobi SVD with the smallest singular value zeroed, denormalised, scaled to Frobenius norm 1, signed so
 *     that its largest-magnitude entry is positive.  The mask is not recomputed from it.  Inliers that allow no such fit (r = 0 among them): no model.
 *   No model never throws pairs away: inliers all 1, f3x3 nine zeros, *best = -1, *n_inliers = n_points, POPPY_OK.  Identical images and pure shifts are
 *     planar-degenerate and may end here.
 *   counts (2048) and models (2048 x 9 doubles, F_h; zeros where invalid) are optional.  POPPY_E_ARG — nothing written — for a null required pointer, n_points
 *   outside 8 .. 65536, or a distance that is negative or not finite.  NaN and infinite coordinates are not pinned.
 * poppy_hip_ransac_fundamental needs no resident pair and disturbs none.                                                                                    */
#define POPPY_RANSAC_HYPOTHESES 2048
#define POPPY_RANSAC_MIN_POINTS 8
#define POPPY_RANSAC_MAX_POINTS 65536
int poppy_ransac_fundamental(const float* points1, const float* points2, int n_points, double distance,
                             uint8_t* inliers, int* n_inliers, double* f3x3, int* best, int* counts, double* models);
int poppy_hip_ransac_fundamental(poppy_hip_ctx* ctx, const float* points1, const float* points2, int n_points, double distance,
                                 uint8_t* inliers, int* n_inliers, double* f3x3, int* best, int* counts, double* models);

/* ---- auto-align (Settings::enable_auto_align) ---------------------------------------------------
 * warp_affine : cv::warpAffine(src, dst, M, src.size()) for 8UC3, INTER_LINEAR, BORDER_CONSTANT 0, M = 2x3 forward map
 *               (OCV/imgproc/src/imgwarp.cpp:2155-2290,2582-2640) — what Transformer::translate / rotate and
 *               reprocrustes apply to corrected2 (src/transformer.cpp:21-30,268).
 * auto_align  : Matcher::autoAlign (src/matcher.cpp:133-244) on a host image and two point lists: image2 and points2 are
 *               replaced by their aligned versions; *distance = morph distance afterwards.
 * align_step  : one Transformer step on the same arguments — 0 retranslate, 1 reprocrustes, 2 rerotate
 *               (src/transformer.cpp:99-217,260-269); *distance = the value the step returns.
 * align_scores: (diagnostics, tests) what the searches of those steps rank their candidates by — morph_distance(points1, set k)
 *               in a width x height image for n_candidates versions of the second point list (sets: n_candidates x n_points
 *               float pairs), scored in one launch.  distances receives the value per candidate; totals, n_pairs and
 *               inner_sums the scoring kernel's three outputs behind it: the float sum of the greedy pairs' distances, the
 *               number of pairs (a set point at exactly (-1, -1) is the reference's "claimed" marker and pairs with nothing)
 *               and the raw float sum of the set's offsets from points1.  Each output may be NULL.
 * The three take 4 .. 4096 point pairs (POPPY_E_ARG otherwise).
 * procrustes / perspective_from4 (host only): Procrustes(true,false)::procrustes (src/procrustes.cpp:52-114; rotation 2x2,
 *               scale_error[2], yprime n x 2) and cv::getPerspectiveTransform of four point pairs (3x3 doubles).
 * poppy_hip_pair_begin runs auto_align itself when settings.enable_auto_align is set.                              */
int poppy_hip_warp_affine(poppy_hip_ctx* ctx, const uint8_t* src, size_t src_stride, int width, int height, const double* m2x3,
                          uint8_t* dst, size_t dst_stride);
int poppy_hip_auto_align(poppy_hip_ctx* ctx, uint8_t* image2, size_t stride, int width, int height,
                         const float* points1, float* points2, int n_points, double* distance);
int poppy_hip_align_step(poppy_hip_ctx* ctx, int which, uint8_t* image2, size_t stride, int width, int height,
                         const float* points1, float* points2, int n_points, double* distance);
int poppy_hip_align_scores(poppy_hip_ctx* ctx, const float* points1, const float* sets, int n_points, int n_candidates, int width, int height,
                           double* distances, float* totals, int* n_pairs, float* inner_sums);
int poppy_procrustes(const float* x, const float* y, int n_points, float* rotation4, float* scale_error2, float* yprime);
int poppy_perspective_from4(const float* src4, const float* dst4, double* m3x3);

/* Matcher::find (general branch) + Matcher::prepare on raw point lists (src/matcher.cpp:118-131,246-332):
 * drop out-of-image pairs, morph distance, greedy nearest-neighbour pairing, threshold filter, 4 corners.
 * Host only.  out1/out2 need room for n_points + 4 pairs.                                              */
/* Self-check of the matcher's hypotf (point_match.cpp): compares its closed form with the libm hypotf the library is linked
 * against on n pseudo-random float pairs; returns the number of mismatches (0 expected).  Host only.                    */
long poppy_hypotf_selfcheck(long n, uint64_t seed);
int poppy_match_points(const float* points1, const float* points2, int n_points, int width, int height,
                       double match_tolerance, float* out1, float* out2, int* n_out, double* initial_morph_distance);

/* Extractor::foreground for ONE image (src/extractor.cpp:136-229; the reference runs it on both images of a pair,
 * three times per pair: poppy.hpp:52,116 and matcher.cpp:17): grey -> 13 x MOG2 on progressively median-blurred copies
 * (k = 1, 9, ..., 89), accumulated and Gaussian-smoothed -> log mask -> x grey -> equalizeHist.  Returns the 8-bit
 * `goodFeatures` image (width*height bytes).  Bit-exact with the reference.  First part of the pre-ORB filter chain
 * (SURVEY 8f-1); poppy_hip_orb_input / poppy_hip_gabor_field are the rest, poppy_hip_pair_begin runs all of it.
 * debug (optional, host pointers, each may be NULL): grey w*h; stages 50 planes of w*h in the order flow0, acc0, then
 * 12 x (med, flow, acc, blur); floats 3 planes of w*h: lin, logged, finalMask; masked w*h.                      */
typedef struct poppy_foreground_debug {
    uint8_t* grey;
    uint8_t* stages;
    float* floats;
    uint8_t* masked;
} poppy_foreground_debug;
int poppy_hip_foreground(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, int width, int height,
                         uint8_t* good_features, const poppy_foreground_debug* debug);
/* One link of that chain on its own: cv::medianBlur(src, dst, ksize) on a tight 8-bit single-channel host image, odd 3 <= ksize <= 89
 * (src/extractor.cpp:149; OCV/imgproc/src/median_blur.simd.hpp:84-346).  form selects the kernel (diagnostics, tests): 0 = what the chain
 * takes for this ksize, 1 = a lane per image column (k_median_u8), 2 = column histograms over the ranks of the values each tile's
 * footprint holds (k_median_cols: one count per lane up to 64 values, two up to 129, windows of 128 ranks beyond), 3 = k_median_cols
 * without the presence maps (every tile by windows over all 256 values), 4 = as 2 without the one-count form, 5 = as 2 with every tile
 * by windows, 6 / 7 = as 5 with the first window at the top / bottom of the ranks (the windows beside it do the work).  All forms return
 * the same bytes.                                                                                                                     */
int poppy_hip_median_blur(poppy_hip_ctx* ctx, const uint8_t* src, int width, int height, int ksize, int form, uint8_t* dst);
/* What tests of those medians need to state what they reach; host only, no result depends on them.
 * poppy_median_cols_geom: how k_median_cols cuts a width x height image: tiles_x x tiles_y tiles of tile_cols columns by rows rows (the last
 * ones cut by the image; POPPY_MED_COLS_ROWS, read once per process, sets rows).  Each pointer may be NULL.
 * poppy_median_cols_hint: the choice between the two median kernels that the set-up makes from a sparse sample of a host BGR image: 1 = its
 * tiles hold few values (the chain takes k_median_cols), 0 = not, or an image under 256 x 64 (k_median_u8).  POPPY_E_ARG (negative) on bad
 * arguments.
 * poppy_hip_foreground_median_links: of the last chain that the context's image slot `which` (0: poppy_hip_foreground and a pair's first
 * image, 1: a pair's second image; a chained next pair swaps them) ran: cols_mask bit i = the median of ksize 8 i + 1 went through
 * k_median_cols (bit 0 never: eleven real links, 0xffe), decided_by = POPPY_MEDIAN_BY_* below, 0 before any chain.                         */
#define POPPY_MEDIAN_BY_HINT 1      /* the host sample (poppy_median_cols_hint) */
#define POPPY_MEDIAN_BY_DEVICE 2    /* the device's count of tiles of at most 24 values: nine tenths of the tiles -> k_median_cols */
#define POPPY_MEDIAN_BY_ENV 3       /* POPPY_MED_COLS_FORCE, or POPPY_MED_COLS_MIN above 89 */
int poppy_median_cols_geom(int width, int height, int* tiles_x, int* tiles_y, int* rows, int* tile_cols);
int poppy_median_cols_hint(const uint8_t* bgr, size_t stride, int width, int height);
int poppy_hip_foreground_median_links(poppy_hip_ctx* ctx, int which, unsigned* cols_mask, int* decided_by);

/* The last stage of every frame on its own: unsharp_mask(src, 1, amount, 0.3) + convertTo(CV_8U, 255) (src/util.cpp:113-148,
 * src/algo.cpp:263-265) on a host float image of width x height BGR pixels, `pitch` pixels per row (>= width; the padding pixels are
 * uploaded with the rows and must not influence the result).  dst: tight 8-bit BGR; dst_f32_or_null: the float image before the 8-bit
 * conversion, tight (what the debug fetch "unsharp" returns for a frame).  The launcher, the threshold and the bound of the decision are
 * the frame path's own.  form selects the kernel (diagnostics, tests): 0 = what a frame of this geometry takes (the POPPY_UNSHARP_STREAM /
 * POPPY_UNSHARP_TILE switches apply), 1 = the tile kernel (k_unsharp_tile; POPPY_E_UNSUPPORTED under 2 pixels wide or high), 2 = the
 * streaming kernel (k_unsharp_stream; POPPY_E_UNSUPPORTED under 64 x 16), 3 = the three separable kernels frames under 2 pixels wide or
 * high take (any geometry).  amount_on_device: 0 = the amount is the kernel's argument, 1 = the kernel reads it from a 4-byte device
 * buffer as the frames of a captured body do (the separable kernels have no such form and take the argument).  All forms return the same
 * bits.  Bad arguments: POPPY_E_ARG, nothing written.                                                                                  */
int poppy_hip_unsharp_frame(poppy_hip_ctx* ctx, const float* src, int width, int height, int pitch, float amount, int form,
                            int amount_on_device, uint8_t* dst, float* dst_f32_or_null);

/* Pair set-up from the two ORB input images g1/g2 (what Extractor::keypoints feeds the detector,
 * src/extractor.cpp:50-78) and gabor2 (src/poppy.hpp:119-122): ORB x2 -> truncate to the shorter list
 * (extractor.cpp:96-99) -> poppy_match_points -> resident pair.  nfeatures = int(max_keypoints * detail).  */
int poppy_hip_pair_begin_prefiltered(poppy_hip_ctx* ctx,
                                     const uint8_t* bgr1, size_t stride1, const uint8_t* bgr2, size_t stride2,
                                     const uint8_t* orb_input1, const uint8_t* orb_input2, const float* gabor2_f32x3,
                                     int width, int height, int nfeatures);
/* Same from the raw BGR pair (the set-up half of poppy::morph, src/poppy.hpp:46-157 with face detection and auto-align
 * off): Extractor::foreground x2 -> dft_detail2 x2 -> nfeatures = int(max_keypoints * 255 / max(d1, d2)) -> unsharp(sigma 2),
 * grey, 31x31 Gabor bank, radial gradient, equalizeHist -> ORB x2 -> matcher -> gabor_filter(image2 / 255) -> resident pair.
 * Parity: bit-exact with the reference end to end (tests/test_gpu_prefilter2.py reproduces the point pairs and frames of
 * the real poppy::morph).  dft_detail2 restates cv::dft operation for operation; the Gabor banks produce the once-rounded
 * exact sums that OpenCV's double-precision DFT correlation yields (DESIGN.md section 7 has the fine print).
 * Frames one pixel wide or high: POPPY_E_UNSUPPORTED before any launch (dft_detail2 keeps an even number of spectrum rows and
 * columns: none of a 1-point DFT, so the reference's detail is 0 / 0 and its nfeatures undefined); the same for poppy_hip_morph,
 * the sharded set-ups and poppy_hip_orb_input's detail.                                                                       */
int poppy_hip_pair_begin(poppy_hip_ctx* ctx, const uint8_t* bgr1, size_t stride1, const uint8_t* bgr2, size_t stride2,
                         int width, int height);
/* poppy_hip_pair_begin with the two raw images already in this GPU's memory (tight rows, width*3 bytes each): the throughput
 * path of a caller whose decoder or previous stage left the images in HBM, and what bench.py times.                      */
int poppy_hip_pair_begin_device(poppy_hip_ctx* ctx, const void* d_bgr1, const void* d_bgr2, int width, int height);
/* The set-up of the NEXT pair of the CLI's loop (src/poppy.cpp:326: img1 = corrected2.clone()): image 1 = the resident pair's second image as
 * poppy::morph hands it back (corrected2, what poppy_hip_pair_corrected2 returns; the ALIGNED image under auto-align), image 2 = bgr.  The same
 * result in every bit as poppy_hip_pair_begin(ctx, corrected2, bgr).  Image 1's filter chain (foreground, dft_detail2, ORB input, the detector's
 * pyramid and FAST candidates, src/extractor.cpp:33-83,136-229) is not run again when it is the image the resident pair's own set-up ran it on:
 * after poppy_hip_pair_begin / _device / _next without auto-align, with no other call in between that filters, detects or replaces the resident
 * images (poppy_hip_render*, _morph_frames, _pair_reset and the frame accessors keep it).  Only nfeatures depends on the pair (quotas, retainBest,
 * Harris, angles: src/extractor.cpp:40-45).  POPPY_E_STATE without a resident pair; POPPY_E_ARG when the size differs from the resident pair's.
 * _device: image 2 in this GPU's memory, tight rows. */
int poppy_hip_pair_begin_next(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, int width, int height);
int poppy_hip_pair_begin_next_device(poppy_hip_ctx* ctx, const void* d_bgr, int width, int height);
/* image chains run and reused by the set-ups of this context since it was created (diagnostic; either pointer may be NULL) */
int poppy_hip_chain_counts(poppy_hip_ctx* ctx, unsigned long long* chains_run, unsigned long long* chains_reused);
/* A poppy_write_cb that only counts: ++*(long long*)user.  For callers (and the benchmark) that want the frame hand-off —
 * every frame downloaded into pinned host memory and presented to the writer — without a consumer of their own.           */
void poppy_count_frames_cb(void* user, const uint8_t* bgr, int width, int height, size_t stride);
/* nfeatures and the two dft_detail2 values of the last poppy_hip_pair_begin */
/* Opt-in quality mode with no counterpart in the reference's live code: pair set-up as poppy_hip_pair_begin, but the point
 * pairs come from ORB descriptors (ORB::compute on both keypoint sets, 2-NN both ways, ratio test, symmetry test) instead of
 * the positional greedy matcher; surviving pairs in query order, out-of-image pairs dropped, four corners appended.
 * POPPY_E_NOMATCH when nothing survives (use poppy_hip_dissolve).  ratio: 0.7 in the reference's sketch.        */
int poppy_hip_pair_begin_descriptors(poppy_hip_ctx* ctx, const uint8_t* bgr1, size_t stride1, const uint8_t* bgr2, size_t stride2,
                                     int width, int height, float ratio);
/* The same with the sketch's third filter: the pairs left after the out-of-image drop go through poppy_hip_ransac_fundamental with this distance (the sketch: 3.0)
 * and only its inliers, still in query order, become the point pairs (then the morph distance and the four corners, as above).  Fewer than 8 pairs: the filter
 * is skipped.  Nothing left before the filter: POPPY_E_NOMATCH.  poppy_hip_pair_fundamental reports what the filter of the resident pair's set-up found: F (nine
 * zeros without a model or when the filter was skipped), the pairs that went in, the pairs that came out and the winning hypothesis (-1 likewise); each pointer may be
 * NULL.  POPPY_E_STATE when the resident pair was set up any other way.                                                                                     */
int poppy_hip_pair_begin_descriptors_ransac(poppy_hip_ctx* ctx, const uint8_t* bgr1, size_t stride1, const uint8_t* bgr2, size_t stride2,
                                            int width, int height, float ratio, double distance);
int poppy_hip_pair_fundamental(poppy_hip_ctx* ctx, double* f3x3, int* n_matches, int* n_inliers, int* best);

/* The second image as the resident pair holds it — after poppy_hip_pair_begin with enable_auto_align this is the ALIGNED
 * corrected2 that poppy::morph hands back to its caller (src/poppy.hpp:46-47; src/poppy.cpp:326 chains it into the next pair). */
int poppy_hip_pair_corrected2(poppy_hip_ctx* ctx, uint8_t* dst, size_t dst_stride);

/* nfeatures = int(max_keypoints * 255 / max(detail2[0], detail2[1])) (src/extractor.cpp:40-45).  Where that quotient is no int (both details 0: two
 * featureless images, whose foregrounds are constant), nfeatures is INT_MIN (-2147483648): what the reference's x86-64 build gets from the conversion
 * (cvttsd2si), written out here.  The detector then keeps every candidate (OCV/features2d/src/keypoint.cpp:69-90 skips retainBest for n < 0);
 * a flat image's ORB input is constant (all 256 grey levels), without any, so such a pair has no point pairs (poppy_hip_morph: POPPY_E_NOMATCH
 * and the dissolve frames).  poppy_hip_orb_detect itself refuses nfeatures < 0.                                                          */
int poppy_hip_pair_begin_info(poppy_hip_ctx* ctx, int* nfeatures, double* detail2);
/* Pieces of the chain, host in / host out, for tests and for callers that cache intermediates:
 * poppy_hip_orb_input: goodFeatures (w*h) -> g = the ORB input image; optional us (grey of the unsharp-masked image), gb (Gabor
 * mean), detail (dft_detail2).  poppy_hip_gabor_field: gabor_filter(bgr / 255) with the default arguments -> f32x3.
 * poppy_radial_gradient: draw_radial_gradiant2 (src/draw.cpp:40-59), host only.  poppy_radial_mask: draw_radial_gradiant + the
 * conversion to float of src/extractor.cpp:181-183 (src/draw.cpp:21-38): the mask enable_radial_mask multiplies in, host only.      */
int poppy_hip_orb_input(poppy_hip_ctx* ctx, const uint8_t* good_features, int width, int height, uint8_t* g, float* us, float* gb, double* detail);
int poppy_hip_gabor_field(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, int width, int height, float* gabor);
/* The two Gabor banks (src/util.cpp:31-61: filter2D per angle -> OCV/imgproc/src/templmatch.cpp:566-760, double-precision DFT
 * correlation) run as tiled double-precision FFTs by default; on != 0 selects the direct double sums instead.  The two forms give the
 * same planes in every bit: the transforms are ~1e-15 from the direct sums before the one rounding to float, and the FFT form hands
 * every pixel with a plane value that close to a float rounding boundary (or to zero) to the direct sums (the tests compare the two).
 * poppy_hip_gabor_doubt (diagnostic): since the last call on the current device, out[0] plane values near zero, out[1] near a
 * midpoint, out[2] pixels formed again because of them. */
int poppy_hip_set_gabor_direct(poppy_hip_ctx* ctx, int on);
int poppy_hip_gabor_doubt(unsigned long long out[3]);
/* How poppy_hip_pair_begin* runs the two images' filter chains (Extractor::foreground -> dft_detail2 -> ORB input -> detector, src/extractor.cpp:33-83, once per image):
 * serial = 0 (default of a context) side by side on two streams and two host threads — the shortest set-up when the context has the GPU to itself —, serial != 0 one
 * after the other.  The contexts of a pool with three or more contexts per device are created with serial = 1: their set-ups run side by side anyway, and six chains on
 * the process's four hardware queues made the pool's speed a lottery.  Both orders leave the same pair state in every bit.                                          */
int poppy_hip_set_setup_chains(poppy_hip_ctx* ctx, int serial);
int poppy_radial_gradient(int width, int height, float* out);
int poppy_radial_mask(int width, int height, float* out);
/* Host-side tables behind two device kernels, exposed for tests that run without a GPU (no reference counterpart):
 * poppy_gabor_tables: the 16 kernels of a Gabor bank as cv::getGaborKernel returns them (which = 31: src/extractor.cpp:63-64, 13:
 * src/util.hpp:95; 16 * which^2 floats) and their paired, conjugated 64 x 64 spectra (8 * 4096 complex doubles) for the FFT form;
 * poppy_pyr_tail_plan: the tap table of the pyramid tail kernel for a frame geometry (info: first tail level, multi-pixel level
 * steps, single-pixel reductions, descriptors, LDS bytes, usable; desc: 4 words per descriptor);
 * poppy_gabor_rounding_in_doubt: the FFT form's doubt rule on one plane value v (the function the kernel calls, run on the host):
 * 0 not in doubt, 1 within band of zero, 2 within band of the midpoint between two floats;
 * poppy_gabor_band_unit: the band the kernels use, per unit of max(1, the largest magnitude in the tile's 64 x 64 patch). */
int poppy_gabor_tables(int which, float* bank, double* spectra);
int poppy_gabor_rounding_in_doubt(double v, double band);
double poppy_gabor_band_unit(void);
int poppy_pyr_tail_plan(int width, int height, int pyramid_levels, int tail_px, int* info, unsigned* desc);
/* Host only: the plan of the length-n transform dft_detail2's kernels run (pass order, load permutation, float twiddles; see
 * poppy_amd/csrc/dft_exact.cpp).  factors needs room for 34 ints, itab for n ints, wave for 2n floats.  For the test suite. */
int poppy_dft_plan(int n, int* factors, int* n_factors, int* itab, float* wave);

/* blur_margin (src/util.cpp:574-602), the CLI's padding step before poppy::morph (src/poppy.cpp:233-240,293-308): the image
 * centred in a union_width x union_height canvas, the four margin strips Gaussian-blurred (127x127, sigma 6).  Bit-exact.
 * POPPY_E_ARG: a null pointer, a non-positive size, a canvas smaller than the image, a stride shorter than its row.
 * POPPY_E_UNSUPPORTED, before anything is allocated or launched and with dst untouched: sizes whose margin strips leave the canvas
 * (poppy_blur_margin_rects below), and a canvas of more rows than the device's grid takes in y (poppy_hip_blur_margin_max_rows).
 * The context stays usable after either.                                                                                       */
int poppy_hip_blur_margin(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, int width, int height,
                          int union_width, int union_height, uint8_t* dst, size_t dst_stride);
/* Host only: the one statement of blur_margin's geometry.  With margin = (width + height) / 100.0 and, per axis,
 * d = |size - union| / 2, then d = (d == 0 ? 1.3 : d + margin):
 *   rects  = left {0, 0, (int)dx, UH}, right {(int)(UW - dx), 0, (int)dx, UH}, top {0, 0, UW, (int)dy}, bottom {0, (int)(UH - dy), UW, (int)dy}
 *            as 16 ints (x, y, width, height), blurred from the unblurred canvas and written in this order (later strips win);
 *   origin = the image's top-left pixel in the canvas, ((int)(|W - UW| / 2), (int)(|H - UH| / 2)).
 * Either pointer may be NULL.  POPPY_E_ARG: a non-positive size or a canvas smaller than the image (nothing written).
 * POPPY_E_UNSUPPORTED (both still written): a strip leaves the canvas, (int)dx > UW or (int)dy > UH — images more than about 99
 * times as high as wide, or as wide as high (8 x 1000 in 10 x 1000).  The reference throws there (Mat(Rect) asserts the rectangle
 * lies inside the matrix); poppy_hip_blur_margin and poppy_hip_morph_list refuse such sizes.
 * A rectangle of width or height 0 (a size difference of 1 with width + height < 100: 3 x 3 in 4 x 4) means "strip skipped".
 * That is this library's rule: the reference's GaussianBlur is never asked about an empty strip by its own CLI.              */
int poppy_blur_margin_rects(int width, int height, int union_width, int union_height, int rects[16], int origin[2]);
/* Host only: blur_margin's 127 fixed-point (8.8) taps, as the strip kernels get them (they sum to 256). */
int poppy_blur_margin_taps(int taps[127]);
/* The most canvas rows poppy_hip_blur_margin and poppy_hip_morph_list's canvas take on this context's device (its maxGridSize[1]). */
int poppy_hip_blur_margin_max_rows(poppy_hip_ctx* ctx, int* rows);

/* --denoise: the CLI's optional fastNlMeansDenoising of every image as it is read (src/poppy.cpp:172), in front of the union size and blur_margin.
 * Non-local means on an 8-bit BGR image with ONE strength hs, in the direct integer form of OpenCV 4.6's fastNlMeansDenoising.  PINNED BY RESTATEMENT
 * ONLY: neither the reference nor OpenCV was at hand, so the rule is DEFINED by the host statement poppy_bgr_denoise below, and poppy_hip_denoise returns
 * the same bytes.  What a fixture from the reference would have to confirm: the constants (fixed_point_mult from 2^32 - 1, the table length, the 0.001
 * cut-off), float evaluation of hs * hs * 3, the border (reflect-101), the rounding of the table and of the final quotient — and the arguments the CLI
 * passes at :172, which SURVEY.md does not record: hs and both windows are arguments here.
 *
 * The rule.  src is width x height; template window tw and search window sw are odd; th = tw / 2, sh = sw / 2, b = th + sh.
 *   1. e = src extended by b on every side with reflect-101, folded as often as needed (a side of 1 maps every index to 0): blur_margin's fold.
 *   2. fpm = min(floor((2^32 - 1) / (sw * sw * 255)), 2^31 - 1); shift = the smallest s with 2^s >= tw * tw; mult = 2^shift / (tw * tw) as a double;
 *      the table has n = (int)(195075 / mult) + 1 entries.
 *   3. den = (hs * hs) * 3 evaluated in FLOAT, then widened to double.  For a = 0 .. n - 1: wd = exp(-(a * mult) / den) in double (the host's libm),
 *      t[a] = round-half-even(fpm * wd), set to 0 where it is below 0.001 * fpm.  The table does not increase; L = the index behind its last non-zero
 *      entry.
 *   4. For pixel (x, y) and every offset (dx, dy) in [-sh, sh]^2:  D = the sum over (i, j) in [-th, th]^2 and the three channels of
 *      (e(x + i, y + j) - e(x + dx + i, y + dy + j))^2.
 *   5. a = D >> shift, wgt = a < L ? t[a] : 0;  est[c] += wgt * e(x + dx, y + dy)[c], ws += wgt, in unsigned 32-bit arithmetic (est <= 255 ws < 2^32 by the
 *      choice of fpm).
 *   6. dst[c] = (est[c] + ws / 2) / ws, where ws / 2 is the integer half and the SUM is not reduced modulo 2^32: at sw = 21 an all-255 image has
 *      est = 4 294 881 360, 85 936 under 2^32, and est + ws / 2 above it; the result is 255.  ws >= t[0] = fpm > 0: the centre offset has D = 0.
 * With tw = 7, sw = 21: fpm = 38192, shift = 6, n = 149355, and L = 143 at hs = 3, 1585 at 10, 6340 at 20, 25357 at 40, the whole table at 100.
 *
 * Refusals, the same in every entry point below, before a byte is read, anything is allocated or launched, and with dst untouched:
 *   POPPY_E_ARG          a null pointer, a non-positive size, a stride shorter than its row, hs not finite or <= 0, an even or non-positive window
 *                        (poppy_hip_denoise_device: also d_src == d_dst);
 *   POPPY_E_UNSUPPORTED  tw outside 3 .. POPPY_DENOISE_MAX_TEMPLATE or sw outside 3 .. POPPY_DENOISE_MAX_SEARCH.  These limits are the kernel's; the host
 *                        statement shares them, so the two agree on what exists.
 * Left out: the per-channel h form (a vector of strengths), fastNlMeansDenoisingColored, grey and 16-bit images, larger windows.                          */
#define POPPY_DENOISE_MAX_TEMPLATE 7
#define POPPY_DENOISE_MAX_SEARCH 21
#define POPPY_DENOISE_TILE_W 58        /* poppy_denoise_tile */
#define POPPY_DENOISE_TILE_H 64
#define POPPY_DENOISE_TABLE_LDS 8192   /* poppy_denoise_table_bound */
/* Host only: the ONE place the weight table and its constants are formed (steps 2 and 3); the GPU path uploads this table and never evaluates exp.
 * table (may be NULL with capacity 0: the constants alone) takes n entries; a capacity below n: POPPY_E_ARG with *n set.  Every output may be NULL. */
int poppy_denoise_weights(float hs, int template_window, int search_window, uint32_t* table, int capacity,
                          int* n, int* L, uint32_t* fixed_point_mult, int* shift);
/* Host only: the rule, from per-offset squared-difference images and their integrals (every D exactly). */
int poppy_bgr_denoise(const uint8_t* bgr, size_t stride, int width, int height, float hs, int template_window, int search_window,
                      uint8_t* dst, size_t dst_stride);
/* Host only: the output tile of the kernel's workgroups, and the longest table prefix L the kernel stages in LDS (a longer one is read from global
 * memory) — for tests, which take their sizes and strengths from here. */
int poppy_denoise_tile(int* tile_width, int* tile_height);
int poppy_denoise_table_bound(int* entries);
/* The same bytes from the GPU.  Host image in, host image out, synchronous; needs no resident pair and disturbs none.  The table of the last
 * (hs, tw, sw) and a staging image are kept by the context. */
int poppy_hip_denoise(poppy_hip_ctx* ctx, const uint8_t* bgr, size_t stride, int width, int height, float hs, int template_window, int search_window,
                      uint8_t* dst, size_t dst_stride);
/* Device image in, device image out, tight rows, d_src != d_dst, queued on poppy_hip_stream(ctx).  (A change of hs or of a window since the last call
 * waits for that stream once, while the table is replaced.) */
int poppy_hip_denoise_device(poppy_hip_ctx* ctx, const uint8_t* d_src, uint8_t* d_dst, int width, int height, float hs, int template_window, int search_window);
/* The CLI's --denoise for poppy_hip_morph_list.  hs = 0 (the default; the windows are ignored): off.  Otherwise the list call denoises EVERY image its
 * source hands it, as it arrives — host or device images, with or without a canvas — at the image's OWN size and in front of the canvas padding
 * (:172 before :239), into buffers of the context: the source's buffer is never written.  The result is the list of the images poppy_bgr_denoise returns
 * with the setting off; each image's filter chain still runs once (poppy_hip_chain_counts does not change).  Bad arguments: refused here, as above, and
 * the setting stays as it was.  The setting is read when a list call starts.
 * Where it does not apply: poppy_hip_morph, the pair loaders (poppy_hip_pair_begin and the rest), the pools and the multi-GPU entry points take their
 * images as they are — the reference's morph never denoises, its run loop does. */
int poppy_hip_set_denoise(poppy_hip_ctx* ctx, float hs, int template_window, int search_window);
int poppy_hip_get_denoise(poppy_hip_ctx* ctx, float* hs, int* template_window, int* search_window);
/* copies of the resident point sets after pair_begin / pair_load (n x 2 floats each); n via *n_points */
int poppy_hip_pair_points(poppy_hip_ctx* ctx, float* points1, float* points2, int max_points, int* n_points);

/* n frames with explicit ratios on the resident pair (frame-range sharding: each GPU renders its own
 * sub-range of phase-mode frames; shape[j] = mask[j] = t_j reproduces morph(..., phase = t_j) with
 * number_of_frames = 1).  chain as in poppy_hip_render.  write may be NULL.                            */
int poppy_hip_render_many(poppy_hip_ctx* ctx, const double* shape_ratio, const double* mask_ratio, int n, int chain,
                          poppy_write_cb write, void* user);

/* ---- multi-GPU (implementation notes in poppy_amd/csrc/rccl_comm.cpp) ----------------------------------------------
 * The path shards by FRAMES of one pair in phase mode (each frame = morph(.., phase = t_j) with number_of_frames = 1,
 * src/poppy.hpp:186-200,234-235) and by PAIRS (the pairs loop of the CLI, src/poppy.cpp:266-328).  The only exchange is the pair
 * state — both images, the mask field's grey complement, the point sets: one contiguous allocation — from the GPU that ran the
 * pair set-up to the others, as ONE ncclBroadcast over RCCL / xGMI.  librccl is loaded on first use.
 *
 * One process per GPU:  comm_id on one rank -> the 128 bytes to the others by any out-of-band channel -> comm_init on every
 * rank's context -> per pair: pair_begin on the root, pair_broadcast everywhere, render_many on every rank's frame range.
 *   comm_id / comm_init / comm_free   ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy for this context's device
 *   pair_broadcast                    the resident pair of `root` becomes the resident pair of every rank (non-root contexts
 *                                     allocate for width x height); with auto-align, phase == 1 on a receiver writes the ALIGNED image
 *   comm_max                          max over the ranks of a host double (step timing)
 *   pair_state_bytes / pair_export_device / pair_import_device   the same packed state to / from a caller's device buffer, for
 *                                     callers with a transport of their own                                                 */
#define POPPY_COMM_ID_BYTES 128
int poppy_hip_comm_id(uint8_t* id128);
int poppy_hip_comm_init(poppy_hip_ctx* ctx, int rank, int world, const uint8_t* id128);
int poppy_hip_comm_free(poppy_hip_ctx* ctx);
/* rank / world as handed to poppy_hip_comm_init, and what the RCCL communicator itself reports (ncclCommUserRank / ncclCommCount; -1 without one):
 * a launcher's check that the job it started is the job the library communicates in (bench.py --gpus N asserts count == N).  Any pointer may be NULL. */
int poppy_hip_comm_info(poppy_hip_ctx* ctx, int* rank, int* world, int* nccl_rank, int* nccl_count);
int poppy_hip_pair_broadcast(poppy_hip_ctx* ctx, int root, int width, int height);
/* The pair set-up ITSELF spread over the communicator's ranks — a collective that replaces poppy_hip_pair_begin_device + poppy_hip_pair_broadcast
 * (the serial part of a sharded morph): rank `root` holds the raw pair (device pointers; the other ranks pass NULL) and filters / detects image 1,
 * rank root + 1 does image 2, rank root + 2 the mask field (src/poppy.hpp:52,114-122: independent until the matcher); the raw pair, the
 * two dft_detail2 values, image 2's keypoint positions, the matched point sets and the mask field's grey complement are exchanged through the
 * communicator.  Afterwards every rank holds the resident pair exactly as poppy_hip_pair_begin_device would have produced it on one GPU
 * (one limit of its own: image 2's keypoints travel through the state's point area, 16 383 at most — far above max_keypoints x detail
 * for every setting of the reference's CLI).  POPPY_E_UNSUPPORTED with enable_auto_align.  Opt-in in poppy_hip_morph_sharded
 * (POPPY_HIP_SHARD_SETUP=1) and bench.py (--shard-setup) until its RCCL transport has run on three or more GPUs.  _local: the same protocol between n contexts of THIS process (host threads; context k = rank k). */
int poppy_hip_pair_begin_sharded(poppy_hip_ctx* ctx, const void* d_bgr1, const void* d_bgr2, int width, int height, int root);
/* How often the sharded protocol itself ran in this process (a world of one takes poppy_hip_pair_begin_device instead unless
 * POPPY_HIP_SHARD_WORLD1 is set): lets a test on a one-GPU box see that the protocol, over RCCL, is what it exercised. */
unsigned long long poppy_hip_sharded_setups(void);
int poppy_hip_pair_begin_sharded_local(poppy_hip_ctx** ctxs, int n, const void* d_bgr1, const void* d_bgr2, int width, int height, int root);
int poppy_hip_comm_max(poppy_hip_ctx* ctx, double* value);
int poppy_hip_pair_state_bytes(int width, int height, size_t* bytes);
int poppy_hip_pair_export_device(poppy_hip_ctx* ctx, void* d_dst, size_t bytes);
int poppy_hip_pair_import_device(poppy_hip_ctx* ctx, const void* d_src, size_t bytes, int width, int height);
/* One process, several GPUs (a drop-in behind the reference's single-process CLI): one host thread + one context per device,
 * communicators from ncclCommInitAll.
 *   morph_sharded  ONE total_frames-frame phase-mode morph of the pair: frame j = morph(img1, img2, .., phase = j / total_frames)
 *                  with number_of_frames = 1 (frame 0 is the phase == 0 copy of image 1); device k renders the k-th contiguous
 *                  share.  `write` is called concurrently from n_devices threads, each with ascending frame indices.
 *   morph_pairs    n_pairs independent pairs, each one whole poppy_hip_morph(.., phase, ..) (default chained mode for phase < 0),
 *                  taken off a shared counter by contexts_per_device host threads per GPU (2-3 fill a GPU: a chained sequence is
 *                  a latency chain, and one pair's set-up runs beside another pair's frames).  `source` hands out pair p's two
 *                  images for the device that will render it (pointers must stay valid until the pair's last frame was written;
 *                  return 0); `write` gets (pair, frame) and is called concurrently.  Both are called from the pool's own threads, never
 *                  from the calling thread.  No communication.
 *   pool_*         the same with contexts (and their HBM) kept between batches; inputs_on_device != 0: `source` returns device
 *                  pointers (tight rows) in the memory of the device it is asked for.
 * err (may be NULL) receives the message of the first failure.                                                              */
typedef struct poppy_hip_pool poppy_hip_pool;
typedef void (*poppy_write_indexed_cb)(void* user, int frame_index, const uint8_t* bgr, int width, int height, size_t stride);
typedef int (*poppy_pair_source_cb)(void* user, int pair_index, int device, const uint8_t** bgr1, size_t* stride1, const uint8_t** bgr2, size_t* stride2);
typedef void (*poppy_write_pair_cb)(void* user, int pair_index, int frame_index, const uint8_t* bgr, int width, int height, size_t stride);
poppy_hip_pool* poppy_hip_pool_create(const int* devices, int n_devices, int contexts_per_device, const poppy_settings* settings,
                                      char* err, size_t err_len);
/* The same, with the start-up check a long-lived service makes once: the contexts of a pool get their streams, hardware queues and buffers from the
 * runtime, and about one pool in ten runs every batch 10-25 % slower for as long as it lives.  Up to max_candidates (1..8) pools are made, each renders a
 * built-in calibration batch of the given geometry (two pairs per context, once untimed, twice timed); two pools that agree within 4 % end the search;
 * the fastest is returned, the others are destroyed.  candidates_ms (may be NULL, room for max_candidates): the batch time of every pool made, in order;
 * *n_made, *kept (may be NULL): how many were made, which one was kept.                                                                             */
poppy_hip_pool* poppy_hip_pool_create_tuned(const int* devices, int n_devices, int contexts_per_device, const poppy_settings* settings,
                                            int width, int height, int max_candidates, float* candidates_ms, int* n_made, int* kept,
                                            char* err, size_t err_len);
void poppy_hip_pool_destroy(poppy_hip_pool* pool);
int poppy_hip_pool_morph_pairs(poppy_hip_pool* pool, int n_pairs, int width, int height, double phase, int inputs_on_device,
                               poppy_pair_source_cb source, poppy_write_pair_cb write, void* user, char* err, size_t err_len);
/* The same batch without waiting for it: poppy_hip_pool_submit_pairs queues it and returns, poppy_hip_pool_wait returns when every pair submitted so far has been
 * rendered and written (the first failure's code and message; the pairs queued behind a failure are dropped).  Batches are taken up in order, pair by pair, by
 * whichever context is free, so the last pairs of one batch render beside the first set-ups of the next — the contexts of a pool fed this way never start a round of
 * set-ups together (the reference's CLI loop over pairs, src/poppy.cpp:266-328, fed by a service instead of a directory listing).  `source`, `write` and `user` must
 * stay valid until the wait.  Do not mix with a poppy_hip_pool_morph_pairs call in flight; poppy_hip_pool_destroy renders what is still queued first.        */
int poppy_hip_pool_submit_pairs(poppy_hip_pool* pool, int n_pairs, int width, int height, double phase, int inputs_on_device,
                                poppy_pair_source_cb source, poppy_write_pair_cb write, void* user);
int poppy_hip_pool_wait(poppy_hip_pool* pool, char* err, size_t err_len);
/* poppy_hip_set_timing / poppy_hip_timing_summary / poppy_hip_warp_counts over all contexts of a pool */
int poppy_hip_pool_set_timing(poppy_hip_pool* pool, int on);
int poppy_hip_pool_timing_summary(poppy_hip_pool* pool, const char** names, float* total_ms, int* launches, int max);
int poppy_hip_pool_warp_counts(poppy_hip_pool* pool, unsigned long long* fused, unsigned long long* tiled, unsigned long long* general);
/* poppy_hip_set_frame_format on every context of the pool; POPPY_E_STATE while batches submitted with poppy_hip_pool_submit_pairs have not been
 * waited for (poppy_hip_pool_wait). */
int poppy_hip_pool_set_frame_format(poppy_hip_pool* pool, int format);
/* poppy_hip_set_frame_scale on every context of the pool; POPPY_E_ARG outside 1..POPPY_FRAME_SCALE_MAX, POPPY_E_STATE as for the format. */
int poppy_hip_pool_set_frame_scale(poppy_hip_pool* pool, int factor);
/* poppy_hip_set_frame_size on every context of the pool; POPPY_E_ARG as there, POPPY_E_STATE as for the format. */
int poppy_hip_pool_set_frame_size(poppy_hip_pool* pool, int ow, int oh);
/* poppy_hip_set_jpeg_quality on every context of the pool; POPPY_E_ARG outside 1..100, POPPY_E_STATE as for the format. */
int poppy_hip_pool_set_jpeg_quality(poppy_hip_pool* pool, int quality);
/* poppy_hip_set_jpeg_budget on every context of the pool; POPPY_E_ARG above 2^32 - 1, POPPY_E_STATE as for the format. */
int poppy_hip_pool_set_jpeg_budget(poppy_hip_pool* pool, size_t max_frame_bytes);
/* poppy_hip_set_jpeg_sequence_budget on every context of the pool; POPPY_E_STATE as for the format. */
int poppy_hip_pool_set_jpeg_sequence_budget(poppy_hip_pool* pool, uint64_t max_sequence_bytes);
/* poppy_hip_mask_rider of the pool's contexts (they share settings and geometry) */
int poppy_hip_pool_mask_rider(poppy_hip_pool* pool);
/* The CLI's loop over an image list (src/poppy.cpp:266-328) on ONE context: pair k = (image k, image k + 1), where image k of pair k > 0 is
 * the corrected2 that pair k - 1 handed back (:326; the aligned image under auto-align).  The same result in every bit as
 *     for k: poppy_hip_morph(ctx, img1, img_{k+1}, .., phase, 0, ..); img1 = corrected2 (poppy_hip_pair_corrected2 when auto-align is on)
 * with pair 0 set up by poppy_hip_pair_begin and every later pair by poppy_hip_pair_begin_next: each image's filter chain runs once
 * (poppy_hip_chain_counts: n_images chains, n_images - 2 of them reused, with auto-align off).
 *   source          called on the calling thread, once per image, in index order: *bgr, *stride, *width, *height of image `image_index`;
 *                   return 0.  The pointer must stay valid until source is called for image index + 2, or until this call returns.
 *                   inputs_on_device != 0: device pointers of this context's GPU, tight rows (*stride is ignored).
 *   canvas          canvas_width = canvas_height = 0: every image must have image 0's size (poppy::morph takes one size,
 *                   src/poppy.cpp:313-316), else POPPY_E_ARG.  Otherwise every image (at most the canvas in each side) is placed into
 *                   the canvas by blur_margin's rule on the device, the bytes poppy_hip_blur_margin(img, canvas) returns (src/util.cpp:574-602).
 *                   An image whose margin strips would leave the canvas (poppy_blur_margin_rects), or a canvas of more rows than
 *                   poppy_hip_blur_margin_max_rows: POPPY_E_UNSUPPORTED when that image arrives, before it is padded; the context stays usable.
 *   denoise         poppy_hip_set_denoise with hs > 0 beforehand (the CLI's --denoise, :172): every image is denoised on the device as it arrives, at
 *                   its own size and in front of the canvas padding, into the context's buffers; the setting is read when the call starts.
 *   phase           < 0: default chained mode; 0 < phase < 1: one phase-mode frame per pair.  0 or 1 with more than two images:
 *                   POPPY_E_UNSUPPORTED (poppy::morph returns before it sets corrected2, :54-70); with two images as poppy_hip_morph.
 *   write           (pair, frame) in order, on the calling thread; NULL keeps the frames on the device.
 *   morph_distances the printed morph distance of every pair (n_images - 1 doubles, may be NULL).
 * The first pair that is not POPPY_OK ends the call with its status, after writing what poppy_hip_morph writes (the linear-blend frames of
 * POPPY_E_NOMATCH); *pairs_done (may be NULL) = the pairs that returned POPPY_OK.  No --distance mode.                                   */
typedef int (*poppy_image_source_cb)(void* user, int image_index, const uint8_t** bgr, size_t* stride, int* width, int* height);
int poppy_hip_morph_list(poppy_hip_ctx* ctx, int n_images, int canvas_width, int canvas_height, double phase, int inputs_on_device,
                         poppy_image_source_cb source, poppy_write_pair_cb write, void* user,
                         double* morph_distances, int* pairs_done);
/* a poppy_write_pair_cb that only counts, atomically: ++*(long long*)user */
void poppy_count_pair_frames_cb(void* user, int pair_index, int frame_index, const uint8_t* bgr, int width, int height, size_t stride);
int poppy_hip_morph_sharded(const int* devices, int n_devices, const poppy_settings* settings,
                            const uint8_t* bgr1, size_t stride1, const uint8_t* bgr2, size_t stride2, int width, int height,
                            int total_frames, poppy_write_indexed_cb write, void* user, char* err, size_t err_len);
int poppy_hip_morph_pairs(const int* devices, int n_devices, int contexts_per_device, const poppy_settings* settings, int n_pairs,
                          int width, int height, double phase, poppy_pair_source_cb source, poppy_write_pair_cb write, void* user,
                          char* err, size_t err_len);

/* File sinks for the frame hand-off, host only, no codec library: poppy_sink_write has the poppy_write_cb signature
 * (user = the sink), so  poppy_hip_morph(ctx, .., poppy_sink_write, sink, ..)  writes the sequence to disk.  RAW: one file, BGR rows back
 * to back; PPM: one P6 file per frame, `path` holds exactly one %d, %<width>d or %0<width>d for the frame index (the library substitutes
 * it itself; any other conversion, or none, makes poppy_sink_open return NULL); Y4M: one YUV4MPEG2 file, C444, full-range BT.601.
 * Y4M420: one YUV4MPEG2 file, C420jpeg XCOLORRANGE=FULL, written from POPPY_FRAME_I420 frames as they come (stride must be the width).
 * GIF: one GIF89a file written from POPPY_FRAME_PAL8 frames as they come (stride must be the width; width, height <= 65535): no global colour
 * table, a NETSCAPE2.0 block that loops forever, and per frame a graphic control extension (delay = fps_den * 100 / fps_num rounded to the
 * nearest centisecond, at least 1), an image descriptor with the frame's palette as a 256-entry local colour table and LZW data (minimum
 * code size 8).  No frame differencing, no transparency.
 * GIF_GLOBAL: as GIF, for POPPY_FRAME_PAL8_SEQ frames: the first frame's palette is written as a 256-entry GLOBAL colour table (logical
 * screen flags 0xF7), a frame whose palette equals it gets an image descriptor without a local table (flags 0x00), and a frame whose
 * palette differs gets its own local table as under GIF (0x87) — so PAL8 frames and the frames of several pairs are taken too and decode
 * to the pixels the GIF sink's file decodes to.  The header goes out with the first frame, which names the table.
 * GIF_CODED: POPPY_SINK_GIF's file from POPPY_FRAME_GIF frames (stride must be 0): header, NETSCAPE2.0 block, and per frame the graphic control extension, the
 * descriptor with a local table, the frame's palette, then the frame's bytes 772 .. total as they are.  Decodes to the pixels the GIF sink's file decodes to; its
 * length is 0.99 - 1.16 times that file's on the measured inputs (every segment of the coded form starts a new table).  A frame of any other format fails this sink, and a coded frame fails every other sink.
 * GIF_GLOBAL_CODED: POPPY_SINK_GIF_GLOBAL's file from coded frames (POPPY_FRAME_GIF_SEQ; stride must be 0): the header waits for the first frame, whose palette becomes the
 * 256-entry global table (flags 0xF7); a frame whose palette equals it gets a descriptor with flags 0x00 and no local table, then its bytes 772 .. total as they
 * are; a frame whose palette differs gets a local table (0x87), so POPPY_FRAME_GIF frames and the frames of several pairs are taken too.  A raster frame fails this
 * sink; no frame at all gives GIF's empty file.
 * MJPEG: one RIFF AVI file written from POPPY_FRAME_JPEG frames as they come (stride must be 0, bytes 4 and 5 FF D8, `total` inside the format's capacity, and the
 * frame's SOF0 must name the sink's width and height): a `hdrl` list with the `avih` main header (dwMicroSecPerFrame = 1000000 * fps_den / fps_num rounded,
 * AVIF_HASINDEX, one stream) and one `strl` list — `strh` with fccType `vids`, fccHandler `MJPG`, dwScale = fps_den, dwRate = fps_num, and `strf`, a 40-byte
 * BITMAPINFOHEADER with 24 bits and compression `MJPG` —, a `movi` list with one `00dc` chunk per frame holding the frame's bytes 4 .. total as they are, padded
 * with a zero byte to even length, and an `idx1` index (AVIIF_KEYFRAME, offsets counted from the `movi` fourcc, the unpadded length).  The RIFF, `movi` and index
 * lengths, the frame counts and the largest chunk's size are patched in at close; no frame at all gives a valid file of no frames.  A frame that would take the
 * file past 4 GiB fails the sink (a plain AVI has 32-bit lengths).  A frame of any other format fails this sink, and a JPEG frame fails every other sink.
 * POPPY_FRAME_JPEG444 frames are taken as well, in any mix with POPPY_FRAME_JPEG frames (the `MJPG` stream does not care): a frame whose SOF0 gives component 1
 * the sampling byte 0x11 is held to POPPY_FRAME_JPEG444's capacity, any other to POPPY_FRAME_JPEG's; nothing else about the sink differs.  POPPY_FRAME_JPEG_OPT
 * and POPPY_FRAME_JPEG444_OPT frames are taken in the same mix: a frame whose DHT segment is not byte for byte the Annex K one is held to the OPT capacity of its
 * sampling, every other frame as before.
 * PNG: one PNG file per frame from POPPY_FRAME_PNG, POPPY_FRAME_PNG_RUNS, POPPY_FRAME_PNG_OPT and POPPY_FRAME_PNG_SEQ frames as they come, in any mix (a PNG file does not say who coded it); `path` follows
 * PPM's %d rule exactly.  The file holds the frame's bytes 4 .. total as they are.  The stride must be 0, bytes 4..11 the PNG signature, IHDR must name the sink's
 * width and height, and `total` must be inside the larger of the two formats' capacities.  A frame
 * of any other format fails this sink, and a PNG frame fails every other sink.
 * The BGR sinks take frames with stride >= 3 * width, the I420 and GIF sinks frames with stride == width: a frame of another format fails the
 * sink where its stride tells (a BGR frame at the I420 or GIF sink, an I420 or PAL8 frame at a BGR sink); a writer must match the context's format.
 * poppy_sink_close returns the number of frames written, or a negative status if a write failed or a frame had another geometry.   */
typedef struct poppy_sink poppy_sink;
enum { POPPY_SINK_RAW = 0, POPPY_SINK_PPM = 1, POPPY_SINK_Y4M = 2, POPPY_SINK_Y4M420 = 3, POPPY_SINK_GIF = 8, POPPY_SINK_GIF_GLOBAL = 16, POPPY_SINK_GIF_CODED = 64, POPPY_SINK_GIF_GLOBAL_CODED = 128, POPPY_SINK_MJPEG = 256, POPPY_SINK_PNG = 1024 };
poppy_sink* poppy_sink_open(const char* path, int format, int width, int height, int fps_num, int fps_den);
void poppy_sink_write(void* sink, const uint8_t* bgr, int width, int height, size_t stride);
int poppy_sink_close(poppy_sink* sink);

/* n frames of the sharded job on the resident pair: frame k = morph(img1, img2, .., phase = t[k]) with number_of_frames = 1, i.e. a
 * copy of image 1 / image 2 for t == 0 / t == 1 (src/poppy.hpp:54-70) and an independent phase-mode frame otherwise.  What a rank
 * renders for its frame range t_j = j / total (poppy_hip_morph_sharded does the same internally).                              */
int poppy_hip_render_phases(poppy_hip_ctx* ctx, const double* t, int n, poppy_write_cb write, void* user);

/* No-match fallback  img2*phase + img1*(1-phase)  (src/poppy.hpp:125-134; u8 addWeighted,
 * OCV/core/src/arithm.simd.hpp:1705-1755).                                                          */
int poppy_hip_dissolve(poppy_hip_ctx* ctx, const uint8_t* img1, size_t stride1, const uint8_t* img2, size_t stride2,
                       int width, int height, double phase, uint8_t* dst, size_t dst_stride);

/* ---- diagnostics: copy an intermediate of the LAST frame to the host (parity tests) -----------
 * names: "triMap"(i32 HxW) "trImg1" "trImg2"(u8 HxWx3) "lbmask"(f32 HxW) "lapBlend" "unsharp"(f32 HxWx3);
 * of the resident pair: "gabor2"(f32 HxWx3, not on ranks that received the pair by broadcast) "m2"(f32 HxW)
 * "unsharp" is only available after poppy_hip_set_debug(ctx, 1).                                       */
int poppy_hip_set_debug(poppy_hip_ctx* ctx, int on);
/* Which warp kernel rendered the last frame: 2 = the fused raster + map + remap kernel (k_warp_bin: triangle ids rasterised per
 * tile in LDS, no id map; the normal case), 1 = the packed-arithmetic kernel on an id map from k_raster (k_warp_tile: debug mode,
 * POPPY_HIP_IDMAP, or a plan whose per-tile lists outgrew the blob), 0 = the general kernel (degenerate matrices or odd
 * geometry).  Same output bits in all three; exported so that the parity tests can tell which one they exercised.           */
int poppy_hip_last_warp_kind(poppy_hip_ctx* ctx);
/* The pyramid launches of the last frame rendered in debug mode, in launch order, as (kind, level, arg) triples in out[3 * k ..]:
 * at most `cap` triples are written; returns how many the frame had (POPPY_E_STATE when no debug frame was rendered since the pair's
 * geometry was set).  The launch sequence depends on the pair's geometry, pyramid_levels and the POPPY_HIP_NOCONE / POPPY_HIP_NOFUSE /
 * POPPY_TAIL_PX switches only, so it also describes the same pair's frames outside debug mode.  Kinds (POPPY_PYR_*):
 *   DOWN    level i -> i + 1 (arg 1: level 0 reads the blend mask from the pair's m2, "lazy", else 0)
 *   DOWN2   levels i -> i + 2 in one launch (k_pyrdown2)
 *   TAIL    k_pyr_tail from level `level` (arg: its multi-pixel steps, n_wide); always followed by
 *   TAIL_NL level = pyramid_levels, arg: the tail's single-pixel reductions (nl; -1 when the pyramid stops above 1 x 1)
 *   MIX_TOP the coarsest level's mix from global memory (the tail does not fit)
 *   CONE    k_collapse_cone<arg> writes level `level` from level + arg
 *   UP2     k_collapse2 writes level `level` from level + 2
 *   UP      level i from i + 1 (arg as for DOWN)
 *   UNSHARP level 0; arg 1: the separable path of frames under 2 pixels wide or high, 0: the 2-D kernels              */
enum { POPPY_PYR_DOWN = 1, POPPY_PYR_DOWN2 = 2, POPPY_PYR_TAIL = 3, POPPY_PYR_TAIL_NL = 4, POPPY_PYR_MIX_TOP = 5, POPPY_PYR_CONE = 6,
       POPPY_PYR_UP2 = 7, POPPY_PYR_UP = 8, POPPY_PYR_UNSHARP = 9 };
int poppy_hip_last_pyramid_forms(poppy_hip_ctx* ctx, int* out, int cap);
/* frames rendered by each of the three since the context was created */
int poppy_hip_warp_counts(poppy_hip_ctx* ctx, unsigned long long* fused, unsigned long long* tiled, unsigned long long* general);
/* Measurement aid: relaunches the last frame's fused raster + warp kernel (create_map + remap, src/algo.cpp:146-176,230-238) `reps`
 * times back to back with nothing else running; *ms_per_launch = time between two events around the batch / reps.  POPPY_E_STATE when
 * the last frame did not take that kernel. */
int poppy_hip_time_last_warp(poppy_hip_ctx* ctx, int reps, float* ms_per_launch);
/* 1 when the warp kernel of this pair also writes the blend mask (lbmask = clamp((1 - mr) - m2 * mr), src/algo.cpp:262-263) beside the
 * two warped images, 0 when the level-0 blend kernels compute it from the pair's m2 field on the values they load (the normal case:
 * 8 B/px per frame less; POPPY_HIP_LBMASK_RIDER=1 or a geometry the wide blend kernels do not take select the former).           */
int poppy_hip_mask_rider(poppy_hip_ctx* ctx);
int poppy_hip_debug_fetch(poppy_hip_ctx* ctx, const char* name, void* host_dst, size_t bytes);
int poppy_hip_debug_triangles(poppy_hip_ctx* ctx, int* n_tris, int* idx3, float* M1, float* M2, int max_tris);

/* Host-only part of one frame (no GPU touched): mesh planning of morph_images, src/algo.cpp:184-228 +
 * the matrix inversions of create_map (:154-157).  Outputs may be NULL.  Used by the CPU test suite.  */
int poppy_plan_frame(int width, int height, const float* src_points1, const float* src_points2, int n_points,
                     double shape_ratio, int max_tris, int* n_tris, int* idx3, int* tri_xy,
                     float* M1, float* M2, float* inv1, float* inv2, float* morphed_pts);

/* Host-only: the lengths of the per-tile triangle lists the fused warp kernels (k_tile_expand, k_warp_bin) would be handed for this
 * frame, in tiles tile_width (64 or 128) pixels wide and 1024 / tile_width high, row-major: the planner's own mesh and binning, with
 * the room for list entries a context keeps for n_points point pairs.  *bins_ok = 0 when the lists outgrow that room (such a frame
 * takes the id-map path); counts[] and *total then hold what the lists would have been.  counts (capacity `cap` tiles), total and
 * bins_ok may be NULL; POPPY_E_ARG when counts is given and *n_tiles > cap.  Used by the CPU test suite.                                            */
int poppy_plan_tile_counts(int width, int height, const float* src_points1, const float* src_points2, int n_points,
                           double shape_ratio, int tile_width, int* counts, int cap, int* n_tiles, long long* total, int* bins_ok);
/* Host-only: the lists themselves, tile after tile in the order of poppy_plan_tile_counts: tris[] (capacity `cap` entries; may be NULL) receives the
 * *total triangle numbers (indices into poppy_plan_frame's triangles), ascending inside a tile, which is painter's order: entry e of a tile's list
 * is what the fused kernels number e + 1 in that tile.  POPPY_E_ARG when *total > cap.  Used by the CPU test suite.                              */
int poppy_plan_tile_tris(int width, int height, const float* src_points1, const float* src_points2, int n_points,
                         double shape_ratio, int tile_width, int* tris, long long cap, long long* total);

/* Host-only: where the groups of a frame's plan lie in a slot's plan blob (poppy_amd/csrc/plan_blob.h), for n_tris triangles, n_work work items of the
 * id-map raster, n_toff tile offsets and n_ttri tile-list entries, on the fused path (fused != 0) or the id-map path: out[0..8] = rec_bytes, o_edges,
 * o_outl, o_toff, o_ttri, o_tri, o_inv, o_work, used, in bytes (the offsets of the group the path does not upload are 0).
 * With capacity != 0 the four counts are instead n_points, width, height and the tile width (64, 128, or 0: what a context picks for that size), and
 * out[0..4] = the bytes a context allocates for a slot's blob with that many point pairs, its triangle budget, its tile count, the tile-list entries it
 * keeps room for, and the tile width; out[5..8] = 0.  Used by the CPU test suite; the library does not call it.                               */
int poppy_plan_blob_layout(int capacity, int n_tris, long long n_work, long long n_toff, long long n_ttri, int fused, unsigned long long* out);

/* Host-only: packs T pairs of inverse matrices (as poppy_plan_frame returns them) into the (T+1) x 20 float records the
 * tiled warp kernel reads (record 0 = identity; layout in poppy_amd/csrc/frame_plan.h) and returns 1 when every matrix is
 * inside the range for which that kernel's arithmetic is proven identical to the general one, 0 when the frame must take
 * the general kernel, < 0 on bad arguments.  Exported for the CPU test suite.                              */
int poppy_warp_records(const float* inv1, const float* inv2, int n_tris, int width, int height, float* records);

/* Per-kernel timing with HIP events recorded on the stream each kernel is launched on.
 *   on = 0  off;
 *   on = 1  around every kernel group of a frame (the frame is then issued launch by launch instead of through its
 *           captured graph, so whole-frame throughput is a little lower while this is on);
 *   on = 2  around the fused map+remap kernel (k_warp_tile / k_warp4) only; the rest of the frame runs as usual.
 * timing_summary drains the streams and returns, per kernel group, the summed duration and the number of
 * launches since the last summary / set_timing call; returns the number of entries written.            */
int poppy_hip_set_timing(poppy_hip_ctx* ctx, int on);
int poppy_hip_timing_summary(poppy_hip_ctx* ctx, const char** names, float* total_ms, int* launches, int max);

#ifdef __cplusplus
}
#endif
#endif /* POPPY_HIP_H_ */
