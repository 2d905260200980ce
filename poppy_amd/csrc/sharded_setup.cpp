// sharded_setup.cpp — the pair set-up itself, spread over the ranks: its stages (setup_sharded at the end is the list of them) and the two entry
// points, over RCCL (rccl_comm.h) and between contexts of one process (local_hub.h).
//
// The set-up is the serial part of a sharded morph (Amdahl: ~5.5 ms on one GPU against 60 frames x 90 us per rank at N = 8).  Its three
// heavy pieces are independent until the matcher (src/poppy.hpp:52,114-122, src/extractor.cpp:33-83); shard_protocol.h: shard_roles):
//   A  image 1: Extractor::foreground -> dft_detail2 -> the ORB input -> ORB::detect        on rank `root`
//   B  image 2: the same                                                                     on rank root + 1
//   C  gabor_filter(corrected2 / 255) -> m2                                                  on rank root + 2 (with B when there are two ranks)
// The exchanges, all through the same transport, in this order on EVERY rank and on every failure path — two reductions, then four broadcasts
// (three when A and B are one rank): a start flag (reduction), the raw pair from `root` (one broadcast of the c1 | c2 region), the two detail
// values (one 3-double max-reduction, which also carries an error flag: nfeatures needs both, src/extractor.cpp:40-45), image 2's keypoint
// positions B -> A (one broadcast through the state's point area; shard_protocol.h: pack_handoff), then the matcher on A and two broadcasts that
// complete the pair state everywhere: header + points from A, m2 from C.
// The transport is abstract so that the role logic can run — and be tested bit for bit — with several contexts of ONE process on one
// GPU (LocalHub: device-to-device copies between the contexts' buffers behind a thread barrier).
#include "local_hub.h"
#include "pair_begin.h"
#include "rccl_comm.h"
#include "shard_protocol.h"
#include <functional>

namespace {

struct Transport {
    int rank = 0, world = 1;
    std::function<int(poppy_hip_ctx*, void*, size_t, int)> bcast;     // in place, device memory, complete on return
    std::function<int(poppy_hip_ctx*, double*, int)> allmax;          // host doubles
};

struct ShardedSetup {                          // one rank's state of one run of the protocol
    poppy_hip_ctx* c; Transport& T; ShardRoles roles; int W, H;
    double d[2] = {0, 0};                      // dft_detail2 of image 1 / 2: this rank's own, then (agree) every rank's
    const uint8_t* orb_in[2] = {nullptr, nullptr};
    SetupStatus role[2];                       // how this rank's parts of stage "run this rank's roles" went: [0] role A, [1] roles B and C
    int nfeatures = 0;
    std::vector<OrbKeyPoint> k[2]; int detect_rc[2] = {0, 0};
    int n2 = -1; std::vector<float> xy2;       // on A: image 2's keypoint positions as they arrived (n2 = -1: none usable)
    std::string own_err;                       // this rank's own reason, kept apart from c->err (adopt_pair_state overwrites that)
    int transport_rc = POPPY_OK;               // a transport error from the hand-off on: remembered, the remaining collectives are still entered
    uint8_t* point_area() const { return c->arena + kPairHeadBytes; }
    static constexpr size_t kPointAreaBytes = 2 * (size_t)kPairMaxPoints * 8;
};

std::atomic<unsigned long long> g_sharded_setups{0};     // protocol runs in this process (poppy_hip_sharded_setups): lets a test see that the protocol, not a shortcut, ran

// Which failures stay inside the protocol.  What can fail on ONE rank (an image, a detection, the matcher) never leaves the others inside a
// collective: it is reported through a reduction (agree), through a count of -1 in the keypoint hand-off or through an invalid header that every
// rank refuses; from the keypoint hand-off on a TRANSPORT error is remembered (transport_rc) while the remaining collectives are still entered
// (and nothing it left in the hand-off area is used).  The first two exchanges (the reductions, the raw pair's broadcast) return at once on a
// transport error: every rank sees the failed collective itself there — RCCL fails a collective on all its ranks, the local hub raises its abort
// flag — so none waits in a later one.  One limit the one-GPU set-up does not have: image 2's keypoints travel through the state's point area, so
// more than kHandoffMaxPoints (16 383) of them fail the set-up (the one-GPU path limits only the MATCHED pairs); max_keypoints x detail stays far
// below that for every setting the reference's CLI accepts.

// One 3-double max-reduction — the two details and an error flag — entered by every rank whatever its own outcome `rc`.  Afterwards either every
// rank goes on, with both details in s.d, or every rank returns: the one that failed its own error, the others `others_msg`.
int agree(ShardedSetup& s, int rc, const char* others_msg) {
    double v[3] = {s.d[0], s.d[1], rc == POPPY_OK ? 0.0 : 1.0};
    const int ra = s.T.allmax(s.c, v, 3);
    if (ra) return ra;
    if (v[2] != 0.0) return rc != POPPY_OK ? rc : fail(s.c, POPPY_E_STATE, others_msg);
    s.d[0] = v[0]; s.d[1] = v[1];
    return POPPY_OK;
}

// Role A's and role B's part of a stage.  A rank that holds both runs B's on the set-up's helper thread beside A's; the device is selected per
// thread, so b is told whether that worked there.  false: the helper thread threw (its what() in c->setup_worker.error()).
template <class PartA, class PartB>
bool run_roles(ShardedSetup& s, PartA&& a, PartB&& b) {
    poppy_hip_ctx* c = s.c;
    if (s.roles.is_a && s.roles.is_b) {
        c->setup_worker.run([&]() { b(hipSetDevice(c->device) == hipSuccess); });
        a();
        return c->setup_worker.wait();
    }
    if (s.roles.is_a) a();
    if (s.roles.is_b) b(true);
    return true;
}

// image i's filter chain (and gabor2 behind image 2's where this rank is C as well), through on return
void chain_image(ShardedSetup& s, int i, bool with_gabor, bool device_ok) {
    poppy_hip_ctx* c = s.c;
    SetupStatus& status = s.role[i];
    if (!device_ok) { status.fail("hipSetDevice failed"); return; }
    hipStream_t st = i ? c->aux_stream : c->stream;
    if (!chain_filter(c, i, i ? c->c2 : c->c1, st, &s.d[i], &s.orb_in[i], status)) return;
    if (with_gabor && !gabor2_into_state(c, chain_fg(c, i), st, status)) return;
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) status.fail(std::string("pair set-up: ") + hipGetErrorString(e));
}

// ---- the stages ---------------------------------------------------------------------------------------------------------------
// 0. buffers everywhere, the raw pair into the root's; the first reduction: nobody enters the raw pair's broadcast unless everybody does
int start_and_agree(ShardedSetup& s, const void* d1, const void* d2) {
    poppy_hip_ctx* c = s.c;
    const size_t bytes = (size_t)s.W * s.H * 3;
    int rc = alloc_pair(c, s.W, s.H);
    if (rc == POPPY_OK) { c->pair_ready = false; c->c2_raw_valid = false; }
    if (rc == POPPY_OK && !c->aux_stream && hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking) != hipSuccess) rc = fail(c, POPPY_E_DEVICE, "hipStreamCreate");
    if (rc == POPPY_OK && s.roles.is_a) {
        if (!d1 || !d2) rc = fail(c, POPPY_E_ARG, "the root has no images");
        else if (hipMemcpyAsync(c->c1, d1, bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
                 hipMemcpyAsync(c->c2, d2, bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
                 hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POPPY_E_DEVICE, "copy of the raw pair");
    }
    return agree(s, rc, "another rank could not start the set-up");
}

// 1. the raw pair to every rank
int share_raw_pair(ShardedSetup& s) {
    poppy_hip_ctx* c = s.c;
    return s.T.bcast(c, c->c1, (size_t)((uint8_t*)c->m2 - c->c1), s.roles.a);
}

// 2. the independent pieces: the filter chains on A and B, gabor2 -> m2 on C.  Nothing returns from here: the outcome goes into the next reduction
void run_own_roles(ShardedSetup& s) {
    poppy_hip_ctx* c = s.c;
    const ShardRoles& r = s.roles;
    if (!run_roles(s, [&]() { chain_image(s, 0, false, true); }, [&](bool device_ok) { chain_image(s, 1, r.is_c, device_ok); }))
        s.role[1].fail("pair set-up helper thread: " + c->setup_worker.error());
    if (r.is_c && !r.is_b) gabor2_into_state(c, c->foreground_b, c->stream, s.role[1]);      // gabor2 alone
    if (r.is_c && s.role[1].rc == POPPY_OK) {                               // m2 = 1 - gray(gabor2), where the frames read the mask field from
        launch_gray_inv(c->gabor2, c->m2, s.W * s.H, c->stream);
        if (hipStreamSynchronize(c->stream) != hipSuccess) s.role[1].fail("m2");
    }
}

// the second reduction: both details to every rank (or every rank out), and nfeatures from them
int agree_on_details(ShardedSetup& s) {
    poppy_hip_ctx* c = s.c;
    const SetupStatus& failed = s.role[0].rc ? s.role[0] : s.role[1];
    int rc = failed.rc;
    if (rc) c->err = failed.msg;
    rc = agree(s, rc, "another rank failed in its part of the set-up");
    if (rc) return rc;
    c->last_detail[0] = s.d[0]; c->last_detail[1] = s.d[1];
    s.nfeatures = c->last_nfeatures = nfeatures_of(c->cfg.max_keypoints, s.d[0], s.d[1]);   // src/extractor.cpp:40-45
    return POPPY_OK;
}

// 3. ORB::detect where the ORB inputs lie.  A failed detection is reported further on: by the hand-off's count (B) or the header (A)
void detect(ShardedSetup& s) {
    poppy_hip_ctx* c = s.c;
    const int W = s.W, H = s.H;
    const bool joined = run_roles(s,
        [&]() { s.detect_rc[0] = c->orb.detect(s.orb_in[0], W, W, H, s.nfeatures, c->stream, s.k[0], true); },
        [&](bool device_ok) { s.detect_rc[1] = device_ok ? c->orb_b.detect(s.orb_in[1], W, W, H, s.nfeatures, c->aux_stream, s.k[1], true) : -2; });
    if (!joined) { s.detect_rc[1] = -1; c->orb_b.err = "pair set-up helper thread: " + c->setup_worker.error(); }
}

// 4. image 2's keypoint positions to A: through the state's point area and one broadcast, or directly where A is B's rank too
void hand_off_keypoints(ShardedSetup& s) {
    poppy_hip_ctx* c = s.c;
    const ShardRoles& r = s.roles;
    if (r.a == r.b) {
        if (r.is_a && s.detect_rc[1] >= 0) { s.xy2 = keypoint_xy(s.k[1]); s.n2 = (int)s.k[1].size(); }
        return;
    }
    if (r.is_b) {
        std::vector<float> words;
        int count = pack_handoff(keypoint_xy(s.k[1]).data(), s.k[1].size(), s.detect_rc[1], words);
        if (count < 0) s.own_err = s.detect_rc[1] < 0 ? "orb_detect (image 2): " + c->orb_b.err
                                                      : "image 2 has more keypoints than the hand-off area holds (" + std::to_string(s.k[1].size()) + " > " + std::to_string(kHandoffMaxPoints) + ")";
        const bool sent = hipMemcpyAsync(s.point_area(), words.data(), words.size() * 4, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
                          hipStreamSynchronize(c->stream) == hipSuccess;
        if (!sent) {                                       // not a return: A and the other ranks are about to enter the broadcast.  Say "failed" through
            count = -1;                                    // the protocol (count -1) if the device still takes a 4-byte write, and go on into the collective
            s.own_err = "keypoint hand-off to the matcher's rank";
            (void)hipMemcpy(s.point_area(), &count, 4, hipMemcpyHostToDevice);
        }
    }
    s.transport_rc = s.T.bcast(c, s.point_area(), ShardedSetup::kPointAreaBytes, r.b);
    if (r.is_a) {
        std::vector<float> words(kHandoffWords);
        const bool got = hipMemcpyAsync(words.data(), s.point_area(), words.size() * 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                         hipStreamSynchronize(c->stream) == hipSuccess;
        // a hand-off broadcast that failed leaves stale words in the area: nothing of it may be used
        if (got && !s.transport_rc) unpack_handoff(words.data(), &s.n2, s.xy2);
        else s.own_err = "keypoint hand-off to the matcher's rank failed";
    }
}

// 5. the matcher on A (host) and the header + points staged there.  Whatever failed on A or B ends as a header every rank refuses
void match_and_stage_header(ShardedSetup& s) {
    poppy_hip_ctx* c = s.c;
    if (!s.roles.is_a) return;
    if (s.detect_rc[0] < 0) s.own_err = "orb_detect (image 1): " + c->orb.err;
    else if (s.n2 < 0 && s.own_err.empty()) s.own_err = "image 2's rank reported a failed detection or too many keypoints";
    bool valid = s.detect_rc[0] >= 0 && s.n2 >= 0;
    if (valid) {
        PointLists pts = extractor_points(s.k[0], s.xy2.data(), (size_t)s.n2);
        int rc = prepare_points(c, pts, s.W, s.H, nullptr);
        if (rc == POPPY_OK) rc = set_points(c, pts.p1.data(), pts.p2.data(), (int)pts.p1.size() / 2);
        if (rc == POPPY_OK) rc = stage_pair_state(c);
        if (rc != POPPY_OK) { valid = false; s.own_err = "matcher / pair state: " + c->err; }
    }
    if (!valid) {                                                           // (adopt_pair_state checks the magic)
        (void)hipMemsetAsync(c->arena, 0, kPairHeadBytes, c->stream);
        (void)hipStreamSynchronize(c->stream);
    }
}

// 6. the pair state completed everywhere — header + points from A, m2 from C — and adopted.  Both broadcasts are entered by every rank whatever
// happened before (a transport error on one rank must not leave the others inside the next one)
int complete_and_adopt(ShardedSetup& s) {
    poppy_hip_ctx* c = s.c;
    int rc = s.T.bcast(c, c->arena, kPairHeadBytes + ShardedSetup::kPointAreaBytes, s.roles.a);
    if (rc && !s.transport_rc) s.transport_rc = rc;
    rc = s.T.bcast(c, c->m2, (size_t)s.W * s.H * 4, s.roles.c);
    if (rc && !s.transport_rc) s.transport_rc = rc;
    if (s.transport_rc) return s.transport_rc;
    rc = adopt_pair_state(c);
    if (rc != POPPY_OK && !s.own_err.empty()) return fail(c, POPPY_E_DEVICE, ("sharded set-up: " + s.own_err).c_str());
    return rc;
}

int setup_sharded(poppy_hip_ctx* c, Transport& T, const void* d1, const void* d2, int W, int H, int root) {
    g_sharded_setups.fetch_add(1);
    chain_touch(c);
    // (refusals that every rank makes alike, before any exchange)
    if (c->cfg.enable_auto_align) return fail(c, POPPY_E_UNSUPPORTED, "the sharded set-up does not take auto-align (image 2 changes after the match)");
    if (!setup_size_ok(W, H)) return fail(c, POPPY_E_UNSUPPORTED, kSetupSizeMsg);
    HIPCHK(c, hipSetDevice(c->device));
    ShardedSetup s{c, T, shard_roles(T.rank, T.world, root), W, H};
    int rc = start_and_agree(s, d1, d2); if (rc) return rc;
    rc = share_raw_pair(s); if (rc) return rc;
    run_own_roles(s);
    rc = agree_on_details(s); if (rc) return rc;
    detect(s);
    hand_off_keypoints(s);
    match_and_stage_header(s);
    return complete_and_adopt(s);
}

const char kLeftMsg[] = "another context left the sharded set-up with an error";

}  // namespace

extern "C" {

unsigned long long poppy_hip_sharded_setups(void) { return g_sharded_setups.load(); }

int poppy_hip_pair_begin_sharded(poppy_hip_ctx* c, const void* d1, const void* d2, int W, int H, int root) {
    if (!c) return POPPY_E_ARG;
    const int rc = comm_require(c); if (rc) return rc;
    if (root < 0 || root >= c->comm_world || W <= 0 || H <= 0) return fail(c, POPPY_E_ARG, "bad root / geometry");
    // a world of one needs no exchange — unless POPPY_HIP_SHARD_WORLD1 asks for the protocol anyway: all three roles on this rank, every
    // broadcast and reduction a real RCCL call on the one-rank communicator (what a box with a single GPU can run of the multi-rank path)
    static const bool world1_protocol = getenv("POPPY_HIP_SHARD_WORLD1") != nullptr;
    if (c->comm_world == 1 && !world1_protocol) return poppy_hip_pair_begin_device(c, d1, d2, W, H);
    Transport T;
    T.rank = c->comm_rank; T.world = c->comm_world;
    T.bcast = comm_broadcast;
    T.allmax = comm_max_n;
    return setup_sharded(c, T, d1, d2, W, H, root);
}

// The same set-up by n contexts of THIS process (one host thread each; the contexts may share a GPU): context k plays rank k, the raw
// pair (device pointers valid for context `root`'s device) ends up resident in every context.  What the multi-rank path does, minus RCCL.
int poppy_hip_pair_begin_sharded_local(poppy_hip_ctx** ctxs, int n, const void* d1, const void* d2, int W, int H, int root) {
    if (!ctxs || n < 1 || n > 64 || root < 0 || root >= n || W <= 0 || H <= 0) return POPPY_E_ARG;
    for (int k = 0; k < n; ++k) if (!ctxs[k]) return POPPY_E_ARG;
    if (n == 1) return poppy_hip_pair_begin_device(ctxs[0], d1, d2, W, H);
    LocalHub hub(n);
    std::vector<int> rcs(n, POPPY_OK);
    auto work = [&](int k) {
        Transport T;
        T.rank = k; T.world = n;
        T.bcast = [&hub, k](poppy_hip_ctx* cc, void* buf, size_t bytes, int r) -> int {      // a device copy from the root context's buffer
            hipError_t e = hipSuccess;
            const bool ok = hub.broadcast_slot(k == r, buf, cc->device, [&](const void* src, int) {
                e = hipMemcpyAsync(buf, src, bytes, hipMemcpyDeviceToDevice, cc->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(cc->stream);
            });
            if (!ok) return fail(cc, POPPY_E_STATE, kLeftMsg);
            return e == hipSuccess ? POPPY_OK : fail(cc, POPPY_E_DEVICE, "local broadcast");
        };
        T.allmax = [&hub, k](poppy_hip_ctx* cc, double* v, int m) -> int { return hub.all_max(k, v, m) ? POPPY_OK : fail(cc, POPPY_E_STATE, kLeftMsg); };
        rcs[k] = setup_sharded(ctxs[k], T, k == root ? d1 : nullptr, k == root ? d2 : nullptr, W, H, root);
        if (rcs[k] != POPPY_OK) hub.abort();                               // nobody waits for a context that has returned
    };
    std::vector<std::thread> th;
    for (int k = 1; k < n; ++k) th.emplace_back(work, k);
    work(0);
    for (auto& t : th) t.join();
    for (int k = 0; k < n; ++k) if (rcs[k] != POPPY_OK && rcs[k] != POPPY_E_STATE) return rcs[k];      // the cause before its echoes
    for (int k = 0; k < n; ++k) if (rcs[k] != POPPY_OK) return rcs[k];
    return POPPY_OK;
}

}  // extern "C"
