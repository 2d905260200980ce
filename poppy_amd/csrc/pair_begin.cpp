// pair_begin.cpp — pair set-up from the raw images (pair_begin.h): what poppy::morph does before its frame loop (src/poppy.hpp:46-160), as a schedule
// (SetupSchedule: which order this call takes, decided in one place) and named stages.  pair_begin_impl at the end is the list of them.
#include "pair_begin.h"
#include "setup_latch.h"
#include <chrono>

namespace {

using SetupClock = std::chrono::steady_clock;
enum class Gabor2At { kAfterAlign, kAtStart, kBehindFirstDetect };

struct SetupSchedule {
    bool reuse;            // image 1 = the resident c2 and slot chain_b still holds its chain state: that chain is not run again
    bool serial;           // one image's chain after the other on the GPU, not side by side
    bool align_first;      // Matcher::find aligns the second image before the match: gabor2 belongs to the ALIGNED image
    bool staged;           // the second host image is uploaded by its own chain's thread on that chain's stream
    bool timing;           // POPPY_SETUP_TIMING: the stages' host wall time on stderr
    Gabor2At gabor2;       // where gabor2 — gabor_filter(second image / 255), src/poppy.hpp:119-122 — is queued; every value computes it exactly once (queue_gabor2)
};

SetupSchedule setup_schedule(const poppy_hip_ctx* c, bool on_device, bool next, float ratio) {
    static const bool first_env = getenv("POPPY_GABOR2_FIRST") != nullptr, serial_env = getenv("POPPY_SETUP_SERIAL") != nullptr,
                      timing_env = getenv("POPPY_SETUP_TIMING") != nullptr;
    SetupSchedule s;
    // image 1's chain state is the one the resident pair's set-up left in slot chain_b (never under auto-align: c2 is then the ALIGNED image)
    s.reuse = next && ratio < 0.f && c->kept_gen == c->chain_gen;
    // Serial: a context of a pool of three or more (three set-ups side by side fill the GPU; two chains each would only put six chains on the process's four
    // hardware queues — which layout a pool of three got was a lottery with a 25 % slower outcome in one pool of four, profiles/r05_notes.md section 6),
    // a caller's choice (poppy_hip_set_setup_chains), or POPPY_SETUP_SERIAL
    s.serial = serial_env || c->setup_serial;
    s.align_first = c->cfg.enable_auto_align != 0 && ratio < 0.f;
    // gabor2 depends on the second raw image alone, not on its chain (and has its own buffers): it goes to the plan-upload stream, idle during a set-up.
    // At the very start, beside the first image's chain, when ONE chain is in flight and there is room beside it (chains one after the other: a pool step of
    // six pairs 56.7 -> 56.0 ms; image 1's chain reused: the same picture) or when POPPY_GABOR2_FIRST asks for it.  With two chains side by side it tripled the
    // first medians' time there (one wave per histogram set, round 3): it then starts behind the FIRST image's FAST kernels, queued by that image's thread —
    // that chain is through earlier than the second's, and gabor2 fills the GPU beside the second chain's tail of small launches (against a start behind
    // the second image's medians: 1080p 3.03 -> 2.96 ms, 4K 8.5 -> 8.1, profiles/r05_notes.md)
    const bool early = first_env || s.reuse || s.serial;
    s.gabor2 = s.align_first ? Gabor2At::kAfterAlign : early ? Gabor2At::kAtStart : Gabor2At::kBehindFirstDetect;
    // Host images: the second image's upload is staged, so the first image's chain — stream-ordered behind its own upload — has the GPU to itself for the
    // length of a copy instead of both chains waiting for both copies
    s.staged = !on_device && !next && !early;
    s.timing = timing_env;
    return s;
}

// POPPY_SETUP_TIMING: host wall time of the set-up's stages, cumulative from `begin` (chains = foreground + detail + ORB input (+ gabor2) of both images;
// detect = the two ORB detections; match = the host matcher; finish = m2 + the pair state)
struct SetupTimes {
    SetupClock::time_point enter = SetupClock::now(), begin;
    double upload = 0, chains = 0, detect = 0, matched = 0, chain_end[2] = {0, 0}, joined = 0, serial[3] = {0, 0, 0}, match[2] = {0, 0}, points_set = 0;
    double at(SetupClock::time_point t) const { return std::chrono::duration<double, std::milli>(t - begin).count(); }
    double now() const { return at(SetupClock::now()); }
    void print(int W, int H, const SetupSchedule& sch) const {
        if (sch.serial) fprintf(stderr, "  chains one after the other: image 1 %.3f ms, image 2 (+ gabor2) %.3f ms\n", serial[1] - serial[0], serial[2] - serial[1]);
        if (points_set > 0) fprintf(stderr, "  match stage: points out of the keypoints %.3f, matcher %.3f, set_points %.3f ms (cumulative)\n", match[0], match[1], points_set);
        fprintf(stderr, "  chains: image 1 through %.3f, image 2 through %.3f, both joined %.3f, gabor2 in place %.3f ms\n", chain_end[0], chain_end[1], joined, chains);
        fprintf(stderr, "pair set-up %dx%d: upload %.3f, chains %.3f, detect %.3f, match %.3f, finish %.3f ms (cumulative); before them (drain + queueing the raw pair's copies) %.3f ms\n",
                W, H, upload, chains, detect, matched, now(), -at(enter));
    }
};

struct PairSetup {                       // one call's state, shared by its two chain threads
    poppy_hip_ctx* c; SetupSchedule sch; int W, H; float ratio;
    const uint8_t* bgr2; size_t s2;      // the second image as the caller gave it (the staged upload reads it)
    int sa, sb;                          // the chain slots of image 1 and image 2
    Details details; UploadKnown c2_upload;
    SetupStatus status[2]; double d[2] = {0, 0};
    std::vector<uint8_t> g[2];           // descriptor mode: the ORB inputs on the host (ORB::compute wants them there)
    std::vector<OrbKeyPoint> k[2];
    int gabor2_queued = 0;               // times queue_gabor2 did its work (on the calling thread, whichever place): 1 when the set-up is through
    SetupTimes t;
    double ransac_distance = -1;         // descriptor mode: >= 0 puts the RANSAC fundamental-matrix filter behind the symmetry test, with this distance
    poppy_hip_ctx::LastFundamental fundamental;      // ... and what it found
};

struct SetupHook {                       // a pool lets one context per device set a pair up at a time (pool.cpp: the set-up gate)
    poppy_hip_ctx* c;
    explicit SetupHook(poppy_hip_ctx* c_) : c(c_) { if (c->setup_hook) c->setup_hook(c->setup_hook_user, c, 1); }
    ~SetupHook() { if (c->setup_hook) c->setup_hook(c->setup_hook_user, c, 0); }
};

// The raw pair into c1 / c2 on c->stream (the staged second image: by its chain).  next: image 1 = the resident c2, ordered before c2 is overwritten on the same stream
int load_raw_pair(PairSetup& p, const uint8_t* bgr1, size_t s1, bool on_device, bool next) {
    poppy_hip_ctx* c = p.c;
    const size_t bytes = (size_t)p.W * p.H * 3;
    if (next || on_device) HIPCHK(c, hipMemcpyAsync(c->c1, bgr1, bytes, hipMemcpyDeviceToDevice, c->stream));
    else { const int rc = upload_image(c, c->c1, bgr1, s1, p.W, p.H); if (rc) return rc; }
    if (on_device) HIPCHK(c, hipMemcpyAsync(c->c2, p.bgr2, bytes, hipMemcpyDeviceToDevice, c->stream));
    else if (!p.sch.staged) return upload_image(c, c->c2, p.bgr2, p.s2, p.W, p.H);
    return POPPY_OK;
}

// gabor2 of the second image into c->gabor2.  Called at each of the three places where it can start; queues it at the schedule's one, so once per set-up:
// kAtStart is always passed, kBehindFirstDetect whenever image 1's chain runs (a reused chain implies kAtStart), kAfterAlign whenever the aligner ran.
// Nothing else queues work on copy_stream, uses setup_ev or waits for c2_up_ev.
bool queue_gabor2(PairSetup& p, Gabor2At at, SetupStatus& s) {
    if (at != p.sch.gabor2) return true;
    poppy_hip_ctx* c = p.c;
    hipStream_t st = c->copy_stream;
    bool concurrent = false;
    switch (at) {
    case Gabor2At::kAfterAlign: st = c->stream; break;                    // behind the aligner's warp of c2
    case Gabor2At::kAtStart: break;                                        // (the raw pair's copies have been waited for)
    case Gabor2At::kBehindFirstDetect:                                     // on the first chain's thread, while the second's is inside the same ForegroundFilter
        concurrent = true;
        if (p.sch.staged) {                                                // c2 is written on the other chain's stream: order copy_stream behind that copy
            if (!p.c2_upload.wait()) return false;                         // (the other chain reports the error)
            if (hipStreamWaitEvent(st, c->c2_up_ev, 0) != hipSuccess) return s.fail("gabor2: stream wait failed");
        }
        if (hipEventRecord(c->setup_ev, c->stream) != hipSuccess || hipStreamWaitEvent(st, c->setup_ev, 0) != hipSuccess) return s.fail("gabor2: stream wait failed");
        break;
    }
    ++p.gabor2_queued;
    return gabor2_into_state(c, chain_fg(c, p.sb), st, s, concurrent);
}

// Front half of image i's chain, on its own thread and stream: (staged upload ->) filter chain -> its detail published -> the detector's first half (-> gabor2)
bool chain_front(PairSetup& p, int i, Publish& publish) {
    poppy_hip_ctx* c = p.c;
    SetupStatus& s = p.status[i];
    const int W = p.W, H = p.H, slot = i ? p.sb : p.sa;
    hipStream_t st = i ? c->aux_stream : c->stream;
    if (i == 0 && p.sch.reuse) { p.d[0] = c->kept_detail; publish.now(); return true; }      // ran in the previous set-up: its detail and its detector's first half are in place
    if (i == 1 && p.sch.staged) {
        // gabor2 reads c2 on copy_stream, queued by the FIRST chain's thread: that thread waits (host) until this upload has been QUEUED and its event recorded, then
        // makes copy_stream wait for the event (device).  (Round 5 had no such edge: gabor2 could read a half-written c2 when the helper thread was late.)
        const bool ok = copy_rows_async(c->c2, (size_t)W * 3, p.bgr2, p.s2, (size_t)W * 3, H, hipMemcpyHostToDevice, st) == hipSuccess && hipEventRecord(c->c2_up_ev, st) == hipSuccess;
        p.c2_upload.known(ok);
        if (!ok) return s.fail("pair_begin: upload of the second image failed");
    }
    const uint8_t* gi = nullptr;
    if (!chain_filter(c, slot, i ? c->c2 : c->c1, st, &p.d[i], &gi, s)) return false;
    publish.now();
    // the detector reads the ORB input where it lies; only ORB::compute wants a host copy
    const hipError_t e = p.ratio >= 0.f ? hipMemcpyAsync(p.g[i].data(), gi, (size_t)W * H, hipMemcpyDeviceToHost, st) : hipSuccess;
    if (e != hipSuccess) return s.fail(std::string("pair_begin: ") + hipGetErrorString(e));
    // the detector's first half needs no nfeatures (which takes BOTH images' detail, src/extractor.cpp:40-45): it follows the chain at once,
    // so the image that is through first does not wait for the other with the GPU half idle
    if (chain_orb(c, slot).detect_begin(gi, W, W, H, st, true) < 0) return s.fail("orb_detect: " + chain_orb(c, slot).err);
    return i != 0 || queue_gabor2(p, Gabor2At::kBehindFirstDetect, s);
}

// Image i's chain.  Side by side, each image's thread goes on to the detector's second half by itself as soon as BOTH details are known: the other image's
// detail is ready long before its own candidates are, so nobody waits for a whole chain.  (One chain after the other: detect_finish_both follows.)
void chain_of(PairSetup& p, int i) {
    poppy_hip_ctx* c = p.c;
    Publish publish{p.details};
    UploadExit upload_exit{p.c2_upload, i == 1 && p.sch.staged};
    if (hipSetDevice(c->device) != hipSuccess) { p.status[i].fail("hipSetDevice failed"); return; }
    if (!chain_front(p, i, publish) || p.sch.serial) return;
    p.details.wait_for(2);
    if (p.status[i ^ 1].rc) return;                                   // the other chain failed (its error is reported)
    OrbDetector& orb = chain_orb(c, i ? p.sb : p.sa);
    if (orb.detect_finish(nfeatures_of(c->cfg.max_keypoints, p.d[0], p.d[1]), i ? c->aux_stream : c->stream, p.k[i]) < 0) p.status[i].fail("orb_detect: " + orb.err);
    p.t.chain_end[i] = p.t.now();
}

int run_chains(PairSetup& p) {
    poppy_hip_ctx* c = p.c;
    if (p.sch.serial) {
        p.t.serial[0] = p.t.now(); chain_of(p, 0);
        p.t.serial[1] = p.t.now(); chain_of(p, 1);
        p.t.serial[2] = p.t.now();
    } else {
        c->setup_worker.run([&p]() { chain_of(p, 1); });
        chain_of(p, 0);
        if (!c->setup_worker.wait()) return fail(c, POPPY_E_DEVICE, ("pair set-up helper thread: " + c->setup_worker.error()).c_str());
    }
    p.t.joined = p.t.now();
    if (p.sch.gabor2 != Gabor2At::kAfterAlign) HIPCHK(c, hipStreamSynchronize(c->copy_stream));       // gabor2 is in place
    for (SetupStatus& s : p.status) if (s.rc) return fail(c, s.rc, s.msg.c_str());
    return POPPY_OK;
}

// the detector's second halves of both images side by side, after chains that ran one after the other
int detect_finish_both(PairSetup& p, int nfeatures) {
    poppy_hip_ctx* c = p.c;
    int r1 = 0, r2 = 0;
    OrbDetector &orb1 = chain_orb(c, p.sa), &orb2 = chain_orb(c, p.sb);
    c->setup_worker.run([&]() { r2 = hipSetDevice(c->device) == hipSuccess ? orb2.detect_finish(nfeatures, c->aux_stream, p.k[1]) : -2; });
    r1 = orb1.detect_finish(nfeatures, c->stream, p.k[0]);
    if (!c->setup_worker.wait()) return fail(c, POPPY_E_DEVICE, ("pair set-up helper thread: " + c->setup_worker.error()).c_str());
    if (r1 < 0 || r2 < 0) return fail(c, POPPY_E_DEVICE, ("orb_detect: " + (r1 < 0 ? orb1.err : orb2.err)).c_str());
    return POPPY_OK;
}

// Opt-in descriptor mode (the reference only sketched it, src/experiments.hpp:14-144): ORB::compute on both keypoint sets, 2-NN Hamming both
// ways, ratio test, symmetry test; the surviving pairs, in query order, become the point sets (out-of-image pairs dropped, the four corners appended).
// No positional re-pairing, no threshold.  With p.ransac_distance >= 0 the sketch's third filter, ransacTest, follows drop_out_of_image: pairs that the RANSAC
// fundamental matrix (ransac_filter) does not keep leave the lists, the others stay in query order; under 8 pairs there is nothing to fit and the filter is skipped.
int descriptor_points(PairSetup& p) {
    poppy_hip_ctx* c = p.c;
    const int W = p.W, H = p.H, n1 = (int)p.k[0].size(), n2 = (int)p.k[1].size();
    std::vector<uint8_t> d1((size_t)n1 * 32), d2((size_t)n2 * 32);
    std::vector<float> rows1((size_t)n1 * 7), rows2((size_t)n2 * 7);
    keypoint_rows7(p.k[0], rows1.data()); keypoint_rows7(p.k[1], rows2.data());
    int r1 = 0, r2 = 0;
    std::thread other([&]() { r2 = hipSetDevice(c->device) == hipSuccess ? c->orb_b.describe(p.g[1].data(), W, W, H, rows2.data(), n2, c->aux_stream, d2.data()) : -2; });
    r1 = c->orb.describe(p.g[0].data(), W, W, H, rows1.data(), n1, c->stream, d1.data());
    other.join();
    if (r1 < 0 || r2 < 0) return fail(c, POPPY_E_DEVICE, ("orb_describe: " + (r1 < 0 ? c->orb.err : c->orb_b.err)).c_str());
    std::vector<int> k12((size_t)n1 * 4), k21((size_t)n2 * 4), sym;
    if (c->orb.hamming_knn2(d1.data(), n1, d2.data(), n2, c->stream, k12.data()) < 0 || c->orb.hamming_knn2(d2.data(), n2, d1.data(), n1, c->stream, k21.data()) < 0)
        return fail(c, POPPY_E_DEVICE, ("hamming_knn2: " + c->orb.err).c_str());
    ratio_symmetry(k12.data(), n1, k21.data(), n2, p.ratio, sym);
    std::vector<P2f> a, b;
    for (size_t i = 0; i + 3 <= sym.size(); i += 3) {
        a.push_back(P2f{p.k[0][sym[i]].x, p.k[0][sym[i]].y});
        b.push_back(P2f{p.k[1][sym[i + 1]].x, p.k[1][sym[i + 1]].y});
    }
    drop_out_of_image(a, b, W, H);
    c->last_descriptor_matches = (int)a.size();
    if (a.empty()) return fail(c, POPPY_E_NOMATCH, "no symmetric descriptor matches");
    if (p.ransac_distance >= 0) {
        auto& f = p.fundamental;
        f.valid = true; f.n_matches = f.n_inliers = (int)a.size(); f.best = -1;
        if (a.size() >= (size_t)POPPY_RANSAC_MIN_POINTS) {
            std::vector<uint8_t> keep(a.size());
            const int rc = ransac_filter(c, (const float*)a.data(), (const float*)b.data(), (int)a.size(), p.ransac_distance, keep.data(), &f.n_inliers, f.f, &f.best, nullptr, nullptr);
            if (rc) return rc;
            size_t m = 0;
            for (size_t i = 0; i < a.size(); ++i) if (keep[i]) { a[m] = a[i]; b[m] = b[i]; ++m; }
            a.resize(m); b.resize(m);
        }
    }
    c->initial_morph_dist = morph_distance_ref(a, b, W, H);
    add_image_corners(a, b, W, H);
    return set_points(c, (const float*)a.data(), (const float*)b.data(), (int)a.size());
}

// Matcher::find's auto-align (src/matcher.cpp:29-32): c2 becomes the aligned image and p2 (n x, y pairs) moves with it; the image as it came in stays
// in c2_raw (what phase == 1 writes); gabor2 is the aligned image's (src/poppy.hpp:116-122 runs after Matcher::find)
int align_second_image(PairSetup& p, PointLists& pts) {
    poppy_hip_ctx* c = p.c;
    const size_t bytes = (size_t)p.W * p.H * 3, n = pts.p1.size() / 2;
    if (n < 4) return fail(c, POPPY_E_UNSUPPORTED, "auto-align needs at least 4 keypoint pairs (the reference reads 4 unconditionally)");
    std::vector<P2f> a(n), b(n);
    memcpy(a.data(), pts.p1.data(), n * 8); memcpy(b.data(), pts.p2.data(), n * 8);
    if (!c->c2_raw) HIPCHK(c, hipMalloc((void**)&c->c2_raw, bytes + 16));
    HIPCHK(c, hipMemcpyAsync(c->c2_raw, c->c2, bytes, hipMemcpyDeviceToDevice, c->stream));
    c->c2_raw_valid = true;
    if (c->aligner.run(c->c2, p.W, p.H, a, b, c->stream, nullptr)) return fail(c, POPPY_E_DEVICE, c->aligner.err.c_str());
    memcpy(pts.p2.data(), b.data(), n * 8);
    SetupStatus s;
    return queue_gabor2(p, Gabor2At::kAfterAlign, s) ? POPPY_OK : fail(c, s.rc, s.msg.c_str());
}

// Pair set-up from the raw images: the pre-ORB filter chain on the GPU, then the same steps as pair_begin_prefiltered.  The two images go through the chain
// independently: one host thread and one stream each, so that the medians of one image run beside the Gabor bank of the other.
// next: the set-up of the next pair of the CLI's loop (src/poppy.cpp:326) — image 1 is the resident pair's c2 (bgr1 unused).
// ransac_distance >= 0 (descriptor mode only): the RANSAC filter behind the symmetry test.
int pair_begin_impl(poppy_hip_ctx* c, const uint8_t* bgr1, size_t s1, const uint8_t* bgr2, size_t s2, int W, int H, float ratio, bool on_device = false, bool next = false,
                    double ransac_distance = -1) {
    if (!c) return POPPY_E_ARG;
    if (next) {
        if (!c->pair_ready) return fail(c, POPPY_E_STATE, "pair_begin_next: no resident pair");
        if (W != c->W || H != c->H) return fail(c, POPPY_E_ARG, "pair_begin_next: the image's size differs from the resident pair's");
        bgr1 = c->c2; s1 = (size_t)W * 3;
    }
    if (!bgr1 || !bgr2 || W <= 0 || H <= 0 || s1 < (size_t)W * 3 || s2 < (size_t)W * 3) return fail(c, POPPY_E_ARG, "bad image arguments");
    if (!setup_size_ok(W, H)) return fail(c, POPPY_E_UNSUPPORTED, kSetupSizeMsg);
    HIPCHK(c, hipSetDevice(c->device));
    PairSetup p{c, setup_schedule(c, on_device, next, ratio), W, H, ratio, bgr2, s2};
    p.ransac_distance = ransac_distance;
    const SetupSchedule& sch = p.sch;
    p.sa = sch.reuse ? c->chain_b : 0; p.sb = 1 - p.sa;
    chain_touch(c);                                               // from here on, nothing is kept until this set-up succeeds
    SetupHook setup_hook(c);
    p.t.enter = SetupClock::now();
    int rc = alloc_pair(c, W, H); if (rc) return rc;
    c->pair_ready = false;
    c->c2_raw_valid = false;
    rc = load_raw_pair(p, bgr1, s1, on_device, next); if (rc) return rc;
    p.t.begin = SetupClock::now();
    if (ratio >= 0.f) { p.g[0].resize((size_t)W * H); p.g[1].resize((size_t)W * H); }
    if (!c->aux_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
    if (!c->setup_ev) HIPCHK(c, hipEventCreateWithFlags(&c->setup_ev, hipEventDisableTiming));
    if (!c->c2_up_ev) HIPCHK(c, hipEventCreateWithFlags(&c->c2_up_ev, hipEventDisableTiming));
    if (sch.staged) p.c2_upload.pending();
    else HIPCHK(c, hipStreamSynchronize(c->stream));              // the raw pair's copies
    p.t.upload = p.t.now();
    SetupStatus early;
    if (!queue_gabor2(p, Gabor2At::kAtStart, early)) return fail(c, early.rc, early.msg.c_str());
    // a ForegroundFilter that two threads are about to use allocates first
    if (sch.gabor2 == Gabor2At::kBehindFirstDetect && (chain_fg(c, p.sb).prepare(W, H) || chain_fg(c, p.sb).prepare2(W, H))) return fail(c, POPPY_E_DEVICE, "foreground buffers");
    if (!on_device) {                                             // which median kernel each image's chain takes: from a sample of the host pixels
        if (!next) chain_fg(c, p.sa).median_cols_hint = median_cols_hint_from_host(bgr1, s1, W, H);
        chain_fg(c, p.sb).median_cols_hint = median_cols_hint_from_host(bgr2, s2, W, H);
    }
    rc = run_chains(p); if (rc) return rc;
    c->chains_run += sch.reuse ? 1 : 2;
    c->chains_reused += sch.reuse ? 1 : 0;
    p.t.chains = p.t.now();
    c->last_detail[0] = p.d[0]; c->last_detail[1] = p.d[1];
    const int nfeatures = c->last_nfeatures = nfeatures_of(c->cfg.max_keypoints, p.d[0], p.d[1]);     // src/extractor.cpp:40-45
    if (sch.serial) { rc = detect_finish_both(p, nfeatures); if (rc) return rc; }
    p.t.detect = p.t.now();
    if (ratio >= 0.f) rc = descriptor_points(p);
    else {
        PointLists pts = extractor_points(p.k[0], keypoint_xy(p.k[1]).data(), p.k[1].size());
        if (sch.align_first) { rc = align_second_image(p, pts); if (rc) return rc; }
        p.t.match[0] = p.t.now();
        rc = prepare_points(c, pts, W, H, &c->setup_worker);
        p.t.match[1] = p.t.now();
        if (rc == POPPY_OK) rc = set_points(c, pts.p1.data(), pts.p2.data(), (int)pts.p1.size() / 2);
        p.t.points_set = p.t.now();
    }
    if (rc) return rc;
    if (p.gabor2_queued != 1) return fail(c, POPPY_E_STATE, "pair set-up: gabor2 was not queued exactly once");
    p.t.matched = p.t.now();
    rc = finish_pair_load(c); if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (ratio < 0.f && !sch.align_first) {                       // image 2's chain state stays for the next pair's image 1 (c2 is that image, unaligned)
        c->chain_b = p.sb;
        c->kept_detail = p.d[1];
        c->kept_gen = c->chain_gen;
    }
    if (sch.timing) p.t.print(W, H, sch);
    c->fundamental = p.fundamental;                              // (set_points ended the previous one's validity)
    return POPPY_OK;
}

}  // namespace

bool chain_filter(poppy_hip_ctx* c, int slot, const uint8_t* d_bgr, hipStream_t st, double* detail, const uint8_t** orb_in, SetupStatus& s) {
    const int W = c->W, H = c->H;
    ForegroundFilter& fg = chain_fg(c, slot);
    const uint8_t* gf = fg.run_device(d_bgr, (size_t)W * 3, W, H, st, nullptr);
    if (!gf) return s.fail("foreground: " + fg.err);
    // dft_detail2 and the ORB input both read goodFeatures: the ORB input's kernels are queued behind dft_detail2's before the host waits for the detail value
    // (until round 4 the chain's stream ran dry twice in mid-chain, at the two read-backs of dft_detail2)
    if (fg.detail_begin(gf, W, H, st)) return s.fail("dft_detail2: " + fg.err);
    *orb_in = fg.orb_input(gf, W, H, 0, st);
    if (!*orb_in) return s.fail("orb_input: " + fg.err);
    if (fg.detail_end(detail)) return s.fail("dft_detail2: " + fg.err);
    return true;
}

bool gabor2_into_state(poppy_hip_ctx* c, ForegroundFilter& fg, hipStream_t st, SetupStatus& s, bool concurrent) {
    std::string own_err;
    const float* gab = fg.gabor_field(c->c2, c->W, c->H, st, concurrent ? &own_err : nullptr);
    if (!gab) return s.fail("gabor_field: " + (concurrent ? own_err : fg.err));
    if (hipMemcpyAsync(c->gabor2, gab, (size_t)c->W * c->H * 12, hipMemcpyDeviceToDevice, st) != hipSuccess) return s.fail("gabor2 copy failed");
    return true;
}

std::vector<float> keypoint_xy(const std::vector<OrbKeyPoint>& k) {
    std::vector<float> xy(k.size() * 2);
    for (size_t i = 0; i < k.size(); ++i) { xy[2 * i] = k[i].x; xy[2 * i + 1] = k[i].y; }
    return xy;
}
void keypoint_rows7(const std::vector<OrbKeyPoint>& k, float* rows) {
    for (size_t i = 0; i < k.size(); ++i) {
        float* o = rows + i * 7;
        o[0] = k[i].x; o[1] = k[i].y; o[2] = k[i].size; o[3] = k[i].angle; o[4] = k[i].response; o[5] = (float)k[i].octave; o[6] = (float)k[i].class_id;
    }
}

// Matcher::match / prepare on the host (poppy_match_points), the sums shared with `helper` when there is one
int match_points_with(Worker* helper, const float* p1, const float* p2, int n, int W, int H, double tol, float* o1, float* o2, int* n_out, double* imd) {
    if (n < 0 || W <= 0 || H <= 0 || !n_out || (n && (!p1 || !p2))) return POPPY_E_ARG;
    std::vector<P2f> a(n), b(n);
    if (n) { memcpy(a.data(), p1, (size_t)n * 8); memcpy(b.data(), p2, (size_t)n * 8); }
    drop_out_of_image(a, b, W, H);
    if (a.empty()) { *n_out = 0; if (imd) *imd = 0; return POPPY_OK; }     // caller falls back to the dissolve (poppy.hpp:125)
    std::vector<PointPair> pairs;
    const double d = morph_distance_pairs(a, b, W, H, pairs, helper);
    if (imd) *imd = d;
    match_and_prepare_from(pairs, a, b, W, H, tol, d);
    *n_out = (int)a.size();
    if (o1) memcpy(o1, a.data(), a.size() * 8);
    if (o2) memcpy(o2, b.data(), b.size() * 8);
    return POPPY_OK;
}

PointLists extractor_points(const std::vector<OrbKeyPoint>& k1, const float* xy2, size_t n2) {
    const size_t n = std::min(k1.size(), n2);
    PointLists pts{keypoint_xy(k1), std::vector<float>(xy2, xy2 + 2 * n)};
    pts.p1.resize(2 * n);
    return pts;
}
int prepare_points(poppy_hip_ctx* c, PointLists& pts, int W, int H, Worker* helper) {
    const size_t n = pts.p1.size() / 2;
    pts.p1.resize((n + 4) * 2); pts.p2.resize((n + 4) * 2);                 // room for the four corners (match_points_with copies its input before it writes)
    int m = 0;
    const int rc = match_points_with(helper, pts.p1.data(), pts.p2.data(), (int)n, W, H, c->cfg.match_tolerance, pts.p1.data(), pts.p2.data(), &m, &c->initial_morph_dist);
    if (rc) return fail(c, rc, "poppy_match_points failed");
    pts.p1.resize((size_t)m * 2); pts.p2.resize((size_t)m * 2);
    return POPPY_OK;
}

extern "C" {

int poppy_hip_pair_begin(poppy_hip_ctx* c, const uint8_t* bgr1, size_t s1, const uint8_t* bgr2, size_t s2, int W, int H) {
    return pair_begin_impl(c, bgr1, s1, bgr2, s2, W, H, -1.f);
}
int poppy_hip_pair_begin_device(poppy_hip_ctx* c, const void* d1, const void* d2, int W, int H) {
    return pair_begin_impl(c, (const uint8_t*)d1, (size_t)W * 3, (const uint8_t*)d2, (size_t)W * 3, W, H, -1.f, true);
}
int poppy_hip_pair_begin_next(poppy_hip_ctx* c, const uint8_t* bgr, size_t stride, int W, int H) {
    return pair_begin_impl(c, nullptr, 0, bgr, stride, W, H, -1.f, false, true);
}
int poppy_hip_pair_begin_next_device(poppy_hip_ctx* c, const void* d_bgr, int W, int H) {
    return pair_begin_impl(c, nullptr, 0, (const uint8_t*)d_bgr, (size_t)W * 3, W, H, -1.f, true, true);
}
int poppy_hip_pair_begin_descriptors(poppy_hip_ctx* c, const uint8_t* bgr1, size_t s1, const uint8_t* bgr2, size_t s2, int W, int H, float ratio) {
    if (!(ratio >= 0.f)) return c ? fail(c, POPPY_E_ARG, "ratio must be >= 0") : POPPY_E_ARG;
    return pair_begin_impl(c, bgr1, s1, bgr2, s2, W, H, ratio);
}
int poppy_hip_pair_begin_descriptors_ransac(poppy_hip_ctx* c, const uint8_t* bgr1, size_t s1, const uint8_t* bgr2, size_t s2, int W, int H, float ratio, double distance) {
    if (!(ratio >= 0.f)) return c ? fail(c, POPPY_E_ARG, "ratio must be >= 0") : POPPY_E_ARG;
    if (!(distance >= 0.0) || !(distance <= 1.7976931348623157e308)) return c ? fail(c, POPPY_E_ARG, "the distance must be finite and >= 0") : POPPY_E_ARG;
    return pair_begin_impl(c, bgr1, s1, bgr2, s2, W, H, ratio, false, false, distance);
}
int poppy_hip_chain_counts(poppy_hip_ctx* c, unsigned long long* run, unsigned long long* reused) {
    if (!c) return POPPY_E_ARG;
    if (run) *run = c->chains_run;
    if (reused) *reused = c->chains_reused;
    return POPPY_OK;
}

// the same set-up from the filtered images: ORB detection on the two ORB inputs, the matcher, then poppy_hip_pair_load with the caller's gabor2
int poppy_hip_pair_begin_prefiltered(poppy_hip_ctx* c, const uint8_t* bgr1, size_t s1, const uint8_t* bgr2, size_t s2,
                                     const uint8_t* g1, const uint8_t* g2, const float* gabor2, int W, int H, int nfeatures) {
    if (!c || !bgr1 || !bgr2 || !g1 || !g2 || !gabor2) return POPPY_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    std::vector<OrbKeyPoint> k1, k2;
    if (c->orb.detect(g1, W, W, H, nfeatures, c->stream, k1) < 0 || c->orb.detect(g2, W, W, H, nfeatures, c->stream, k2) < 0) {
        c->err = "orb_detect: " + c->orb.err;
        return POPPY_E_DEVICE;
    }
    PointLists pts = extractor_points(k1, keypoint_xy(k2).data(), k2.size());
    const int rc = prepare_points(c, pts, W, H, nullptr);
    if (rc) return rc;
    return poppy_hip_pair_load(c, bgr1, s1, bgr2, s2, gabor2, W, H, pts.p1.data(), pts.p2.data(), (int)pts.p1.size() / 2);
}

}  // extern "C"
