// morph_sharded.cpp — one process, several GPUs, ONE pair: poppy_hip_morph_sharded runs one host thread and one context per device, each
// rendering a contiguous share of the job's phase-mode frames from the same pair state (rccl_comm.cpp says why that needs no collective
// on the data path).
#include "rccl_comm.h"

extern "C" {

// ONE total_frames-frame phase-mode morph (frame j = morph(img1, img2, ..., phase = j / total_frames) with number_of_frames = 1;
// frame 0 is the phase == 0 copy of image 1) rendered by n_devices GPUs, device k taking the k-th contiguous share.
int poppy_hip_morph_sharded(const int* devices, int n_devices, const poppy_settings* settings, const uint8_t* bgr1, size_t s1,
                            const uint8_t* bgr2, size_t s2, int W, int H, int total_frames, poppy_write_indexed_cb write, void* user,
                            char* err, size_t err_len) {
    if (!devices || n_devices < 1 || n_devices > 64 || !bgr1 || !bgr2 || W <= 0 || H <= 0 || total_frames < 1) { set_err(err, err_len, "bad arguments"); return POPPY_E_ARG; }
    poppy_settings cfg;
    if (settings) cfg = *settings; else poppy_settings_default(&cfg);
    cfg.number_of_frames = 1;
    std::vector<poppy_hip_ctx*> ctx(n_devices, nullptr);
    auto cleanup = [&]() { for (poppy_hip_ctx* c : ctx) if (c) { poppy_hip_comm_free(c); poppy_hip_destroy(c); } };
    for (int k = 0; k < n_devices; ++k) {
        ctx[k] = poppy_hip_create(devices[k], &cfg);
        if (!ctx[k]) { set_err(err, err_len, std::string("poppy_hip_create: ") + poppy_hip_create_error()); cleanup(); return POPPY_E_DEVICE; }
    }
    if (n_devices > 1) {
        std::string why;
        const int rc = comm_init_all(ctx.data(), devices, n_devices, &why);
        if (rc != POPPY_OK) { set_err(err, err_len, why); cleanup(); return rc; }
    }
    // Several devices: the set-up runs on device 0 before any other device's thread exists (nobody can be left waiting inside RCCL when it
    // fails) and the pair state is broadcast.  POPPY_HIP_SHARD_SETUP=1 spreads the set-up itself over the devices instead
    // (poppy_hip_pair_begin_sharded: image 1 on device 0, image 2 on device 1, the mask field on device 2; not under auto-align): opt-in
    // until its RCCL transport has run on a node with three or more GPUs (round-3 advisor finding; the role logic is tested through the
    // in-process transport, the transport through a world of one).
    static const bool shard_on = getenv("POPPY_HIP_SHARD_SETUP") && atoi(getenv("POPPY_HIP_SHARD_SETUP")) != 0;
    const bool shard_setup = n_devices > 1 && !cfg.enable_auto_align && shard_on;
    uint8_t* d_raw = nullptr;
    const size_t P3 = (size_t)W * H * 3;
    if (shard_setup) {
        hipError_t e = hipSetDevice(devices[0]);
        if (e == hipSuccess) e = hipMalloc((void**)&d_raw, 2 * P3);
        if (e == hipSuccess) e = hipMemcpy2D(d_raw, (size_t)W * 3, bgr1, s1, (size_t)W * 3, H, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy2D(d_raw + P3, (size_t)W * 3, bgr2, s2, (size_t)W * 3, H, hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_err(err, err_len, std::string("upload of the raw pair: ") + hipGetErrorString(e)); if (d_raw) (void)hipFree(d_raw); cleanup(); return POPPY_E_DEVICE; }
    } else {
        int rc = poppy_hip_pair_begin(ctx[0], bgr1, s1, bgr2, s2, W, H);
        if (rc == POPPY_OK && ctx[0]->pts1_0.empty()) rc = fail(ctx[0], POPPY_E_NOMATCH, "no point pairs");
        if (rc != POPPY_OK) { set_err(err, err_len, std::string("pair set-up: ") + poppy_hip_last_error(ctx[0])); cleanup(); return rc; }
    }
    std::vector<int> rcs(n_devices, POPPY_OK);
    struct Relay { poppy_write_indexed_cb write; void* user; int base; };
    // A device thread that fails before or inside the collectives must not leave the others waiting in RCCL for ever: it aborts every
    // communicator of the job once (comm_abort: ncclCommAbort makes pending and later operations on it return an error, and FREES the communicator).
    // What the guard gives (comm_guard.h): a device thread that enters a collective later finds no communicator and fails with POPPY_E_STATE; one that
    // is handing the pointer to RCCL at this moment is waited for, so RCCL is not given a freed handle; one that waits for its stream inside a
    // collective holds nothing and is what the abort exists to unblock.  What it does not give: the wait ends after kCommAbortBoundMs, and the abort
    // then goes ahead with a thread still inside RCCL's enqueue call — noted in the job's error text.
    std::once_flag abort_once;
    std::atomic<bool> abort_undrained{false};
    auto abort_all = [&]() {
        std::call_once(abort_once, [&]() {
            for (int k = 0; n_devices > 1 && k < n_devices; ++k)
                if (!comm_abort(ctx[k])) abort_undrained = true;
        });
    };
    std::atomic<int> past_setup{0};
    auto work = [&](int k) {
        poppy_hip_ctx* c = ctx[k];
        int rc = POPPY_OK;
        if (shard_setup) {
            rc = poppy_hip_pair_begin_sharded(c, k == 0 ? d_raw : nullptr, k == 0 ? d_raw + P3 : nullptr, W, H, 0);
            if (rc == POPPY_OK && c->pts1_0.empty()) rc = fail(c, POPPY_E_NOMATCH, "no point pairs");      // every rank sees the same (empty) point sets
        } else if (n_devices > 1) rc = poppy_hip_pair_broadcast(c, 0, W, H);
        // (POPPY_E_NOMATCH is every device's outcome at once, after its last collective: nothing to unblock)
        if (rc != POPPY_OK && rc != POPPY_E_NOMATCH && past_setup.load() < n_devices) abort_all();      // the exchanges are over once every device is past this point
        past_setup.fetch_add(1);
        const int lo = (int)((long long)total_frames * k / n_devices), hi = (int)((long long)total_frames * (k + 1) / n_devices);
        if (rc == POPPY_OK && hi > lo) {
            Relay relay{write, user, lo};
            poppy_write_cb cb = write ? +[](void* u, const uint8_t* bgr, int w, int h, size_t stride) {
                Relay* r = (Relay*)u;
                r->write(r->user, r->base++, bgr, w, h, stride);
            } : (poppy_write_cb) nullptr;
            std::vector<double> t(hi - lo);
            for (int j = lo; j < hi; ++j) t[j - lo] = (double)j / (double)total_frames;      // t_0 = 0: a copy of image 1 (src/poppy.hpp:54-62)
            rc = poppy_hip_render_phases(c, t.data(), hi - lo, cb, &relay);
        }
        rcs[k] = rc;
    };
    std::vector<std::thread> th;
    for (int k = 1; k < n_devices; ++k) th.emplace_back(work, k);
    work(0);
    for (auto& t : th) t.join();
    if (d_raw) { (void)hipSetDevice(devices[0]); (void)hipFree(d_raw); }
    int rc = POPPY_OK;
    for (int k = 0; k < n_devices; ++k)
        if (rcs[k] != POPPY_OK) {
            rc = rcs[k];
            set_err(err, err_len, "device " + std::to_string(devices[k]) + ": " + poppy_hip_last_error(ctx[k]) +
                                  (abort_undrained ? " (the abort did not wait for a thread that was still entering a collective)" : ""));
            break;
        }
    cleanup();
    return rc;
}

}  // extern "C"
