// pool.cpp — one process, several GPUs, MANY pairs: pools of contexts (poppy_hip_pool_*), their set-up gate, and batches of independent pairs
// handed in synchronously (poppy_hip_pool_morph_pairs) or queued (poppy_hip_pool_submit_pairs / poppy_hip_pool_wait).  No communication at all.
#include "context.h"
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>

extern "C" {

// The pairs loop of the reference's CLI (src/poppy.cpp:266-328) over several GPUs: independent pairs, each one whole
// poppy::morph (default chained mode unless phase says otherwise), handed out one at a time to contexts_per_device host threads
// per GPU — a chained sequence is a latency chain that leaves most of a GPU idle, and the pair set-up of one pair runs beside the
// frames of another.  The pool keeps its contexts (and their HBM) between batches.
struct poppy_hip_pool {
    std::vector<poppy_hip_ctx*> ctx;
    std::vector<int> device_of;
    // The set-up gate (round 6): at most `setup_gate` contexts of a device run a pair set-up at a time (0: no gate).  A set-up takes the whole GPU whatever runs
    // beside it; contexts that all start one at once — a batch of as many pairs as contexts — then all render at once, and the copy link idles for the length of
    // the set-up round; set-ups side by side also slow each other (each takes the whole GPU).  One at a time: a pair's frames stream out while the next pair sets up.
    int setup_gate = 0, contexts_per_device = 1;
    std::mutex gate_mu;
    std::condition_variable gate_cv;
    std::map<int, int> setups_running;           // per device
    // Batches handed in without waiting for them (poppy_hip_pool_submit_pairs / poppy_hip_pool_wait): one persistent feeder thread per context takes pairs off the
    // queue's first batch, so a batch's last pairs render beside the next batch's first set-ups — the contexts never start a round of set-ups together.
    struct Batch {
        int n_pairs = 0, W = 0, H = 0, inputs_on_device = 0, taken = 0;
        double phase = -1.0;
        poppy_pair_source_cb source = nullptr; poppy_write_pair_cb write = nullptr; void* user = nullptr;
    };
    std::mutex q_mu;
    std::condition_variable q_cv, q_idle;
    std::deque<std::shared_ptr<Batch>> queue;    // batches with pairs nobody has taken yet
    long long outstanding = 0;                   // pairs submitted and not finished
    bool unwaited = false;                       // a batch was submitted since the last poppy_hip_pool_wait
    int async_rc = POPPY_OK;                     // the first failure since the last poppy_hip_pool_wait (the pairs behind it are dropped)
    std::string async_err;
    std::vector<std::thread> feeders;
    bool quit = false;
};

static void pool_setup_hook(void* user, poppy_hip_ctx* c, int begin);

poppy_hip_pool* poppy_hip_pool_create(const int* devices, int n_devices, int contexts_per_device, const poppy_settings* settings,
                                      char* err, size_t err_len) {
    if (!devices || n_devices < 1 || n_devices > 64 || contexts_per_device < 1 || contexts_per_device > 16) { set_err(err, err_len, "bad arguments"); return nullptr; }
    poppy_hip_pool* p = new poppy_hip_pool();
    p->contexts_per_device = contexts_per_device;
    {   // POPPY_POOL_SETUPS: set-ups side by side per device (0 = as many as contexts).  Default from three contexts on: ONE — six contexts, 36 pairs in one call 7.0-7.5k -> 7.8k
        // frames/s, four contexts 7.0-7.2k -> 7.4k, the bench's batches of six pairs 6.3-6.6k -> 6.7k; two or three at a time: in between (profiles/r06_gate.txt)
        static const int forced = getenv("POPPY_POOL_SETUPS") ? atoi(getenv("POPPY_POOL_SETUPS")) : -1;
        p->setup_gate = forced >= 0 ? forced : (contexts_per_device >= 3 ? 1 : 0);
        if (p->setup_gate >= contexts_per_device) p->setup_gate = 0;
    }
    for (int d = 0; d < n_devices; ++d)
        for (int k = 0; k < contexts_per_device; ++k) {
            poppy_hip_ctx* c = poppy_hip_create(devices[d], settings);
            if (!c) { set_err(err, err_len, std::string("poppy_hip_create: ") + poppy_hip_create_error()); poppy_hip_pool_destroy(p); return nullptr; }
            // (pair_begin.cpp: from three contexts on the chains of a pair run one after the other — six chains on four hardware queues were a lottery, profiles/r05_notes.md
            // section 6; still the better form behind the set-up gate: profiles/r06_gate.txt; POPPY_POOL_CHAINS=0 / 1 forces side by side / serial)
            static const int chains_env = getenv("POPPY_POOL_CHAINS") ? atoi(getenv("POPPY_POOL_CHAINS")) : -1;
            c->setup_serial = chains_env >= 0 ? chains_env != 0 : contexts_per_device >= 3;
            if (p->setup_gate > 0) { c->setup_hook = pool_setup_hook; c->setup_hook_user = p; }
            p->ctx.push_back(c); p->device_of.push_back(devices[d]);
        }
    return p;
}

void poppy_hip_pool_destroy(poppy_hip_pool* p) {
    if (!p) return;
    {                                                              // batches still queued are rendered first (their writers expect every frame)
        std::unique_lock<std::mutex> lk(p->q_mu);                  // (`feeders` is written under q_mu by the first submit: read it there too)
        p->q_idle.wait(lk, [&] { return p->outstanding == 0; });
        p->quit = true;
    }
    p->q_cv.notify_all();
    for (std::thread& t : p->feeders) t.join();
    for (poppy_hip_ctx* c : p->ctx) poppy_hip_destroy(c);
    delete p;
}

// The set-up gate: every pair set-up of a pool's contexts — from host images (poppy_hip_morph) or from resident ones (poppy_hip_pair_begin_device) — passes through here
// (context.h: setup_hook, called by pair_begin.cpp at the set-up's beginning and end)
static void pool_setup_hook(void* user, poppy_hip_ctx* c, int begin) {
    poppy_hip_pool* p = static_cast<poppy_hip_pool*>(user);
    const int dev = c->device;
    if (begin) {
        std::unique_lock<std::mutex> g(p->gate_mu);
        p->gate_cv.wait(g, [&] { return p->setups_running[dev] < p->setup_gate; });
        ++p->setups_running[dev];
    } else {
        { std::lock_guard<std::mutex> g(p->gate_mu); --p->setups_running[dev]; }
        p->gate_cv.notify_all();
    }
}

// one pair of a batch on context wk: the pair source, the set-up (behind the pool's gate), the frames
static int pool_render_pair(poppy_hip_pool* p, int wk, int pi, int W, int H, double phase, int inputs_on_device,
                            poppy_pair_source_cb source, poppy_write_pair_cb write, void* user) {
    poppy_hip_ctx* c = p->ctx[wk];
    struct Relay { poppy_write_pair_cb write; void* user; int pair; int frame; };
    const uint8_t *a = nullptr, *b = nullptr; size_t sa = 0, sb = 0;
    int rc = source(user, pi, p->device_of[wk], &a, &sa, &b, &sb) == 0 ? POPPY_OK : POPPY_E_ARG;
    if (rc != POPPY_OK) c->err = "the pair source failed";
    Relay relay{write, user, pi, 0};
    poppy_write_cb cb = write ? +[](void* u, const uint8_t* bgr, int w, int h, size_t stride) {
        Relay* r = (Relay*)u;
        r->write(r->user, r->pair, r->frame++, bgr, w, h, stride);
    } : (poppy_write_cb) nullptr;
    if (rc == POPPY_OK && !inputs_on_device) rc = poppy_hip_morph(c, a, sa, b, sb, W, H, phase, 0, cb, &relay, nullptr);
    else if (rc == POPPY_OK) {                              // the same call sequence on images that are already in this GPU's memory
        rc = poppy_hip_pair_begin_device(c, a, b, W, H);           // (behind the pool's set-up gate: pool_setup_hook)
        if (rc == POPPY_OK && c->pts1_0.empty()) rc = fail(c, POPPY_E_UNSUPPORTED, "no point pairs: the fallback needs the images on the host (poppy_hip_morph)");
        if (rc == POPPY_OK) rc = poppy_hip_morph_frames(c, phase, cb, &relay);
    }
    return rc;
}

// Batches of pairs: the batch is queued and the call returns; poppy_hip_pool_wait returns when every pair submitted so far has
// been rendered and handed to its writer.  Batches are taken up in submission order, pair by pair, by whichever context is free — a batch's last pairs run beside the
// next batch's first set-ups.  `source`, `write` and `user` must stay valid until the wait; they are called from the pool's threads.
// After a failure the pairs still queued are dropped and the wait reports the first error ("pair N: ..."); a pair without matches (POPPY_E_NOMATCH) got its fallback
// frames and is no error of the batch.
static void pool_feeder(poppy_hip_pool* p, int wk) {
    for (;;) {
        std::shared_ptr<poppy_hip_pool::Batch> b;
        int pi = 0;
        bool drop = false;
        {
            std::unique_lock<std::mutex> lk(p->q_mu);
            p->q_cv.wait(lk, [&] { return p->quit || !p->queue.empty(); });
            if (p->queue.empty()) return;                           // (quit)
            b = p->queue.front();
            pi = b->taken++;
            if (b->taken >= b->n_pairs) p->queue.pop_front();
            drop = p->async_rc != POPPY_OK;
        }
        int rc = POPPY_OK;
        std::string thrown;
        if (!drop) {
            // (an exception on a pool thread — std::bad_alloc is the one that can happen — must reach the waiter as a status: nobody else would decrement `outstanding`)
            try { rc = pool_render_pair(p, wk, pi, b->W, b->H, b->phase, b->inputs_on_device, b->source, b->write, b->user); }
            catch (const std::exception& e) { rc = POPPY_E_DEVICE; thrown = e.what(); }
            catch (...) { rc = POPPY_E_DEVICE; thrown = "unknown exception"; }
        }
        {
            std::lock_guard<std::mutex> lk(p->q_mu);
            if (rc != POPPY_OK && rc != POPPY_E_NOMATCH && p->async_rc == POPPY_OK) {
                p->async_rc = rc;
                p->async_err = "pair " + std::to_string(pi) + ": " + (thrown.empty() ? std::string(poppy_hip_last_error(p->ctx[wk])) : "exception on a pool thread: " + thrown);
            }
            if (--p->outstanding == 0) p->q_idle.notify_all();
        }
    }
}

int poppy_hip_pool_submit_pairs(poppy_hip_pool* p, int n_pairs, int W, int H, double phase, int inputs_on_device,
                                poppy_pair_source_cb source, poppy_write_pair_cb write, void* user) {
    if (!p || n_pairs < 0 || !source || W <= 0 || H <= 0) return POPPY_E_ARG;
    if (!p->ctx.empty() && p->ctx[0]->cfg.enable_auto_align && n_pairs > 1) return POPPY_E_UNSUPPORTED;     // (poppy_hip_pool_morph_pairs says why)
    if (n_pairs == 0) return POPPY_OK;
    auto b = std::make_shared<poppy_hip_pool::Batch>();
    b->n_pairs = n_pairs; b->W = W; b->H = H; b->phase = phase; b->inputs_on_device = inputs_on_device;
    b->source = source; b->write = write; b->user = user;
    {
        std::lock_guard<std::mutex> lk(p->q_mu);
        if (p->feeders.empty())
            for (int k = 0; k < (int)p->ctx.size(); ++k) p->feeders.emplace_back(pool_feeder, p, k);
        p->outstanding += n_pairs;
        p->unwaited = true;
        p->queue.push_back(std::move(b));
    }
    p->q_cv.notify_all();
    return POPPY_OK;
}

int poppy_hip_pool_wait(poppy_hip_pool* p, char* err, size_t err_len) {
    if (!p) { set_err(err, err_len, "bad arguments"); return POPPY_E_ARG; }
    std::unique_lock<std::mutex> lk(p->q_mu);
    p->q_idle.wait(lk, [&] { return p->outstanding == 0; });
    const int rc = p->async_rc;
    p->unwaited = false;
    if (rc != POPPY_OK) set_err(err, err_len, p->async_err);
    p->async_rc = POPPY_OK;
    p->async_err.clear();
    return rc;
}

// The synchronous form: one batch submitted and waited for.  (Not to be mixed with batches of poppy_hip_pool_submit_pairs that nobody has waited for yet: the wait
// is for every pair submitted so far and reports the first failure among them.)
int poppy_hip_pool_morph_pairs(poppy_hip_pool* p, int n_pairs, int W, int H, double phase, int inputs_on_device,
                               poppy_pair_source_cb source, poppy_write_pair_cb write, void* user, char* err, size_t err_len) {
    if (!p || n_pairs < 0 || !source || W <= 0 || H <= 0) { set_err(err, err_len, "bad arguments"); return POPPY_E_ARG; }
    // With auto-align the reference's pairs are NOT independent: the aligned second image of one pair is the first image of the next
    // (src/poppy.cpp:326: img1 = corrected2.clone()), which a caller's pair source cannot know in advance.  Such a sequence is a chain:
    // poppy_hip_morph pair after pair on one context, feeding poppy_hip_pair_corrected2 forward (include/poppy_hip_shim.hpp does).
    if (!p->ctx.empty() && p->ctx[0]->cfg.enable_auto_align && n_pairs > 1) {
        set_err(err, err_len, "enable_auto_align chains the pairs (src/poppy.cpp:326): render them in sequence with poppy_hip_morph, not through the pool");
        return POPPY_E_UNSUPPORTED;
    }
    const int rc = poppy_hip_pool_submit_pairs(p, n_pairs, W, H, phase, inputs_on_device, source, write, user);      // (refuses nothing that was not refused above)
    return rc != POPPY_OK ? rc : poppy_hip_pool_wait(p, err, err_len);
}

// A pool whose contexts came out well.  The contexts of a pool get their streams, hardware queues and buffers from the runtime when they are made, and about
// one pool in ten then runs every batch 10 - 25 % slower for as long as it lives.  What a service does about that once, at start-up, is done
// here: up to max_candidates pools are made, each renders a small calibration batch (a built-in synthetic pair of the given geometry, two pairs per context, the
// frames handed to a counting writer) once untimed and twice timed; the fastest pool is returned, the others are destroyed.  Two pools that agree within 4 %
// end the search — that is the normal state.  candidates_ms (may be NULL, room for max_candidates) receives the timed batch time of every pool made, in the
// order they were made; *n_made their number; *kept the index of the one returned.
namespace {
void calibration_pair(int W, int H, std::vector<uint8_t>& a, std::vector<uint8_t>& b) {
    // flat rectangles on grey, the second image's shifted by a few pixels: corners for the detector, plateaus like the bench's own content
    a.assign((size_t)W * H * 3, 96); b = a;
    auto hash = [](uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; };
    for (uint32_t k = 0; k < 40; ++k) {
        const int w = 24 + (int)(hash(k * 7 + 1) % (uint32_t)std::max(8, W / 10)), h = 24 + (int)(hash(k * 7 + 2) % (uint32_t)std::max(8, H / 10));
        const int x0 = (int)(hash(k * 7 + 3) % (uint32_t)std::max(1, W - w - 16)), y0 = (int)(hash(k * 7 + 4) % (uint32_t)std::max(1, H - h - 16));
        const int dx = 2 + (int)(hash(k * 7 + 5) % 7), dy = 2 + (int)(hash(k * 7 + 6) % 7);
        const uint32_t col = hash(k * 7);
        for (int im = 0; im < 2; ++im) {
            std::vector<uint8_t>& img = im ? b : a;
            const int ox = x0 + (im ? dx : 0), oy = y0 + (im ? dy : 0);
            for (int y = oy; y < std::min(oy + h, H); ++y)
                for (int x = ox; x < std::min(ox + w, W); ++x) {
                    uint8_t* px = &img[((size_t)y * W + x) * 3];
                    px[0] = (uint8_t)col; px[1] = (uint8_t)(col >> 8); px[2] = (uint8_t)(col >> 16);
                }
        }
    }
}
}  // namespace

poppy_hip_pool* poppy_hip_pool_create_tuned(const int* devices, int n_devices, int contexts_per_device, const poppy_settings* settings, int W, int H,
                                            int max_candidates, float* candidates_ms, int* n_made, int* kept, char* err, size_t err_len) {
    if (n_made) *n_made = 0;
    if (kept) *kept = -1;
    if (W <= 0 || H <= 0 || max_candidates < 1 || max_candidates > 8) { set_err(err, err_len, "bad arguments"); return nullptr; }
    std::vector<uint8_t> a, b;
    calibration_pair(W, H, a, b);
    struct Src { const uint8_t *a, *b; size_t stride; long long frames; } src{a.data(), b.data(), (size_t)W * 3, 0};
    auto source = +[](void* u, int, int, const uint8_t** p1, size_t* s1, const uint8_t** p2, size_t* s2) { Src* s = (Src*)u; *p1 = s->a; *p2 = s->b; *s1 = *s2 = s->stride; return 0; };
    auto count = +[](void* u, int, int, const uint8_t*, int, int, size_t) { __atomic_fetch_add(&((Src*)u)->frames, 1ll, __ATOMIC_RELAXED); };
    std::vector<std::pair<poppy_hip_pool*, double>> made;
    auto drop_all = [&]() { for (auto& m : made) poppy_hip_pool_destroy(m.first); };
    for (int k = 0; k < max_candidates; ++k) {
        poppy_hip_pool* p = poppy_hip_pool_create(devices, n_devices, contexts_per_device, settings, err, err_len);
        if (!p) { drop_all(); return nullptr; }
        const int batch = 2 * (int)p->ctx.size();
        int rc = poppy_hip_pool_morph_pairs(p, batch, W, H, -1.0, 0, source, count, &src, err, err_len);      // allocates
        const auto t0 = std::chrono::steady_clock::now();
        for (int q = 0; q < 2 && rc == POPPY_OK; ++q) rc = poppy_hip_pool_morph_pairs(p, batch, W, H, -1.0, 0, source, count, &src, err, err_len);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / 2;
        if (rc != POPPY_OK) { poppy_hip_pool_destroy(p); drop_all(); return nullptr; }
        made.emplace_back(p, ms);
        if (candidates_ms) candidates_ms[k] = (float)ms;
        if (made.size() >= 2) {
            std::vector<double> t;
            for (auto& m : made) t.push_back(m.second);
            std::sort(t.begin(), t.end());
            if (t[0] * 1.04 >= t[1]) break;
        }
    }
    size_t best = 0;
    for (size_t k = 1; k < made.size(); ++k) if (made[k].second < made[best].second) best = k;
    for (size_t k = 0; k < made.size(); ++k) if (k != best) poppy_hip_pool_destroy(made[k].first);
    if (n_made) *n_made = (int)made.size();
    if (kept) *kept = (int)best;
    return made[best].first;
}

int poppy_hip_pool_set_timing(poppy_hip_pool* p, int on) {
    if (!p) return POPPY_E_ARG;
    for (poppy_hip_ctx* c : p->ctx) poppy_hip_set_timing(c, on);
    return POPPY_OK;
}
// per-kernel-group totals summed over the pool's contexts (same contract as poppy_hip_timing_summary)
int poppy_hip_pool_timing_summary(poppy_hip_pool* p, const char** names, float* total_ms, int* launches, int max) {
    if (!p) return 0;
    int n = 0;
    for (poppy_hip_ctx* c : p->ctx) {
        const char* nm[32]; float ms[32]; int cnt[32];
        const int k = poppy_hip_timing_summary(c, nm, ms, cnt, 32);
        for (int i = 0; i < k; ++i) {
            int j = 0;
            while (j < n && strcmp(names[j], nm[i]) != 0) ++j;
            if (j == n) { if (n >= max) continue; names[n] = nm[i]; total_ms[n] = 0.f; launches[n] = 0; ++n; }
            total_ms[j] += ms[i]; launches[j] += cnt[i];
        }
    }
    return n;
}
int poppy_hip_pool_warp_counts(poppy_hip_pool* p, unsigned long long* fused, unsigned long long* tiled, unsigned long long* general) {
    if (!p) return POPPY_E_ARG;
    unsigned long long a = 0, b = 0, f = 0;
    for (poppy_hip_ctx* c : p->ctx) { a += c->n_warp_fast; b += c->n_warp_general; f += c->n_warp_bin; }
    if (fused) *fused = f;
    if (tiled) *tiled = a;
    if (general) *general = b;
    return POPPY_OK;
}

// the body of the pool's four writer setters: refused while work is outstanding (the feeders' contexts may be rendering), then `set` on every context
static int pool_set(poppy_hip_pool* p, const std::function<int(poppy_hip_ctx*)>& set) {
    {
        std::lock_guard<std::mutex> lk(p->q_mu);
        if (p->unwaited || p->outstanding) return POPPY_E_STATE;
    }
    for (poppy_hip_ctx* c : p->ctx) { const int rc = set(c); if (rc) return rc; }
    return POPPY_OK;
}

int poppy_hip_pool_set_frame_format(poppy_hip_pool* p, int format) {
    if (!p || !format_traits(format)) return POPPY_E_ARG;
    return pool_set(p, [=](poppy_hip_ctx* c) { return poppy_hip_set_frame_format(c, format); });
}

int poppy_hip_pool_set_jpeg_quality(poppy_hip_pool* p, int quality) {
    if (!p || quality < 1 || quality > 100) return POPPY_E_ARG;
    return pool_set(p, [=](poppy_hip_ctx* c) { return poppy_hip_set_jpeg_quality(c, quality); });
}

int poppy_hip_pool_set_jpeg_budget(poppy_hip_pool* p, size_t max_frame_bytes) {
    if (!p || max_frame_bytes > 0xffffffffull) return POPPY_E_ARG;
    return pool_set(p, [=](poppy_hip_ctx* c) { return poppy_hip_set_jpeg_budget(c, max_frame_bytes); });
}

int poppy_hip_pool_set_jpeg_sequence_budget(poppy_hip_pool* p, uint64_t max_sequence_bytes) {
    if (!p) return POPPY_E_ARG;
    return pool_set(p, [=](poppy_hip_ctx* c) { return poppy_hip_set_jpeg_sequence_budget(c, max_sequence_bytes); });
}

int poppy_hip_pool_set_frame_scale(poppy_hip_pool* p, int factor) {
    if (!p || factor < 1 || factor > POPPY_FRAME_SCALE_MAX) return POPPY_E_ARG;
    return pool_set(p, [=](poppy_hip_ctx* c) { return poppy_hip_set_frame_scale(c, factor); });
}

int poppy_hip_pool_set_frame_size(poppy_hip_pool* p, int ow, int oh) {
    if (!p || ow < 0 || oh < 0 || (ow == 0) != (oh == 0)) return POPPY_E_ARG;
    return pool_set(p, [=](poppy_hip_ctx* c) { return poppy_hip_set_frame_size(c, ow, oh); });
}

int poppy_hip_pool_mask_rider(poppy_hip_pool* p) {
    if (!p || p->ctx.empty()) return POPPY_E_ARG;
    return poppy_hip_mask_rider(p->ctx[0]);
}

int poppy_hip_morph_pairs(const int* devices, int n_devices, int contexts_per_device, const poppy_settings* settings, int n_pairs,
                          int W, int H, double phase, poppy_pair_source_cb source, poppy_write_pair_cb write, void* user,
                          char* err, size_t err_len) {
    poppy_hip_pool* p = poppy_hip_pool_create(devices, n_devices, contexts_per_device, settings, err, err_len);
    if (!p) return POPPY_E_DEVICE;
    const int rc = poppy_hip_pool_morph_pairs(p, n_pairs, W, H, phase, 0, source, write, user, err, err_len);
    poppy_hip_pool_destroy(p);
    return rc;
}

void poppy_count_pair_frames_cb(void* user, int, int, const uint8_t*, int, int, size_t) {
    if (user) __atomic_fetch_add((long long*)user, 1ll, __ATOMIC_RELAXED);
}

}  // extern "C"
