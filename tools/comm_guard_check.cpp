// comm_guard_check.cpp — the host-only pieces of the multi-GPU code alone, under a sanitizer: the communicator guard (poppy_amd/csrc/comm_guard.h),
// the in-process transport's hub (local_hub.h) and the sharded set-up's role table and keypoint hand-off (shard_protocol.h):
//   clang++ -std=c++17 -O1 -g -DPOPPY_COMM_ABORT_BOUND_MS=20 -fsanitize=thread -pthread tools/comm_guard_check.cpp -o /tmp/guard_tsan && /tmp/guard_tsan
//   clang++ -std=c++17 -O1 -g -DPOPPY_COMM_ABORT_BOUND_MS=20 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread tools/comm_guard_check.cpp -o /tmp/guard_asan && /tmp/guard_asan
// The bound is compiled down (-D) so that the case that outlasts it takes milliseconds.  Every case runs under an alarm: a thread left waiting is a failure too.
#include "../poppy_amd/csrc/comm_guard.h"
#include "../poppy_amd/csrc/local_hub.h"
#include "../poppy_amd/csrc/shard_protocol.h"
#include <climits>
#include <csignal>
#include <cstdio>
#include <memory>
#include <unistd.h>

using namespace poppy_hip;

static const char* g_case = "";
static void hung(int) {
    const char msg[] = "FAILED: a thread was left waiting in case: ";
    (void)!write(2, msg, sizeof msg - 1); (void)!write(2, g_case, strlen(g_case)); (void)!write(2, "\n", 1);
    _exit(2);
}
static void begin_case(const char* name) { g_case = name; alarm(120); }     // (a case takes a second or two; under the thread sanitizer a few more)

// ---- the guard: users against an aborter that frees the object --------------------------------------------------------------
constexpr int kUsers = 3;
struct Comm { int touched[kUsers] = {}; };             // plain ints, one per user: a touch after the delete is a report of either sanitizer

static int guard_rounds(int rounds) {
    begin_case("guard");
    int wrong = 0, late = 0, used = 0;                   // used: rounds in which a user got the pointer before the abort took it
    for (int k = 0; k < rounds; ++k) {
        CommHandle h;
        Comm* obj = new Comm;
        h.set(obj);
        std::atomic<bool> taken{false};
        std::atomic<int> bad{0}, got{0};
        std::thread users[kUsers];
        for (int u = 0; u < kUsers; ++u)
            users[u] = std::thread([&, u] {
                for (int nulls = 0; nulls < 3;) {
                    const bool after = taken.load();
                    CommUse use(h);
                    if (!use.comm) { ++nulls; continue; }
                    if (after || nulls) ++bad;                              // an enter after the take gave the pointer
                    ++static_cast<Comm*>(use.comm)->touched[u];
                    ++got;
                    if (taken.load()) ++bad;                                // inside a bracket after the take returned drained
                }
            });
        for (volatile int spin = (k * 37) % 60000; spin > 0;) spin = spin - 1;      // the abort at varying moments of the users' loops
        bool drained = false;
        void* p = h.take_for_abort(&drained);
        if (p != obj || !h.aborted() || h.present()) ++wrong;
        if (drained) { taken = true; delete obj; }                          // what ncclCommAbort does with the communicator
        else ++late;                                                        // a user descheduled inside its bracket for longer than the (compiled-down) bound
        for (std::thread& t : users) t.join();
        if (!drained) delete obj;
        if (h.enter() || !h.aborted()) ++wrong;
        h.clear_aborted();
        if (h.aborted()) ++wrong;
        wrong += bad.load();
        used += got.load() != 0;
    }
    // a bracket here is two instructions long, so a round that outlasts the bound is the scheduler's doing and rare; a guard whose count never drained
    // would make every round late
    if (late * 100 > rounds) ++wrong;
    if (used * 4 < rounds) ++wrong;                                         // the abort must meet users at work, not only threads that have not started
    printf("%-64s %d rounds, %d wrong (users at work in %d; %d outlasted the %d ms bound)\n", "guard: users against an aborter that frees", rounds, wrong, used, late, kCommAbortBoundMs);
    return wrong;
}

static int guard_bound() {
    begin_case("guard bound");
    CommHandle h;
    auto obj = std::make_unique<Comm>();
    h.set(obj.get());
    std::atomic<bool> inside{false}, release{false};
    std::thread user([&] {
        CommUse use(h);
        inside = true;
        while (!release.load()) std::this_thread::yield();                  // longer than the bound: until the abort has given up on it
        ++static_cast<Comm*>(use.comm)->touched[0];                         // (the object is not deleted in this case)
    });
    while (!inside.load()) std::this_thread::yield();
    bool drained = true;
    const auto t0 = std::chrono::steady_clock::now();
    void* p = h.take_for_abort(&drained);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    release = true;
    user.join();
    const int wrong = (p != obj.get()) + drained + (ms < kCommAbortBoundMs) + !h.aborted() + (h.enter() != nullptr);
    printf("%-64s returned after %.1f ms, drained = %d, %d wrong\n", "guard: a user that outlasts the bound", ms, (int)drained, wrong);
    return wrong;
}

// ---- the hub ------------------------------------------------------------------------------------------------------------------
enum AbortAt { kNever, kBefore, kBetween, kInside };
constexpr int kPhases = 6;

static int hub_rounds(const char* name, int n, int rounds, AbortAt at) {
    begin_case(name);
    int wrong = 0;
    for (int k = 0; k < rounds; ++k) {
        LocalHub hub(n);
        std::vector<int> bufs(n, 0), done(n, 0), bad(n, 0);
        auto work = [&](int rank) {
            const bool aborter = at != kNever && rank == n - 1;
            for (int ph = 0; ph < kPhases; ++ph) {
                if (aborter && (at == kBefore || (at == kBetween && ph == 3))) { hub.abort(); return; }
                const int root = ph % n;
                bool ok;
                if (ph % 2 == 0) {
                    if (rank == root) bufs[rank] = 100 * ph + root;
                    int seen = -1, seen_device = -1;
                    ok = hub.broadcast_slot(rank == root, &bufs[rank], 7 + rank, [&](const void* src, int device) {
                        seen = *(const int*)src; seen_device = device;
                        if (aborter && at == kInside && ph >= 2) hub.abort();      // (in the first broadcast from phase 2 on whose root it is not)
                    });
                    if (ok && rank != root && (seen != 100 * ph + root || seen_device != 7 + root)) ++bad[rank];
                } else {
                    double v[3] = {(double)(rank + ph), (double)-rank, 2.5};
                    ok = hub.all_max(rank, v, 3);
                    if (ok && (v[0] != n - 1 + ph || v[1] != 0.0 || v[2] != 2.5)) ++bad[rank];
                }
                if (!ok) return;
                ++done[rank];
            }
        };
        std::vector<std::thread> th;
        for (int r = 1; r < n; ++r) th.emplace_back(work, r);
        work(0);
        for (std::thread& t : th) t.join();
        for (int r = 0; r < n; ++r) {
            wrong += bad[r];
            // After an abort every other thread comes back with false, and exactly in the phase the aborter did not complete: the phases before it, which
            // every thread reached, stay complete however late a waiter wakes up.  (The aborter itself is one phase behind where it left from inside a phase.)
            int inside = 2;                                                // kInside: the first broadcast (even phase) from phase 2 on whose root is not the aborter, rank n - 1
            while (inside % n == n - 1) inside += 2;
            const int stop = at == kNever ? kPhases : at == kBefore ? 0 : at == kBetween ? 3 : inside;
            if (done[r] != stop) ++wrong;
        }
    }
    printf("%-64s %d rounds, %d wrong\n", name, rounds, wrong);
    return wrong;
}

// ---- the role table and the hand-off --------------------------------------------------------------------------------------------
static int roles_table() {
    int wrong = 0, rows = 0;
    for (int world = 1; world <= 4; ++world)
        for (int root = 0; root < world; ++root)
            for (int rank = 0; rank < world; ++rank, ++rows) {
                const ShardRoles r = shard_roles(rank, world, root);
                const int b = world == 1 ? root : (root + 1) % world, c = world <= 2 ? b : (root + 2) % world;
                if (r.a != root || r.b != b || r.c != c || r.is_a != (rank == root) || r.is_b != (rank == b) || r.is_c != (rank == c)) ++wrong;
                if (world == 1 && !(r.a == r.b && r.b == r.c)) ++wrong;
                if (world == 2 && !(r.b == r.c && r.b != r.a)) ++wrong;
                if (world >= 3 && (r.a == r.b || r.b == r.c || r.a == r.c)) ++wrong;
            }
    printf("%-64s %d rows, %d wrong\n", "shard_roles: worlds 1 to 4, every root and rank", rows, wrong);
    return wrong;
}

static int handoff_case(size_t n, int detect_rc, int want) {
    std::vector<float> xy(2 * n), sent, got;
    for (size_t i = 0; i < xy.size(); ++i) xy[i] = 0.25f * (float)i;
    int wrong = pack_handoff(xy.data(), n, detect_rc, sent) != want;
    wrong += sent.size() != 2 + 2 * (size_t)(want < 0 ? 0 : want);
    std::vector<float> area(kHandoffWords, -7.f);                           // the point area as the matcher's rank reads it back: stale words behind what was sent
    memcpy(area.data(), sent.data(), sent.size() * 4);
    int n2 = 12345;
    unpack_handoff(area.data(), &n2, got);
    wrong += n2 != want;
    if (want >= 0) wrong += got.size() != 2 * n || (n && memcmp(got.data(), xy.data(), got.size() * 4) != 0);
    else wrong += !got.empty();
    return wrong;
}
static int handoff() {
    static_assert(kHandoffMaxPoints == 16383 && kPairMaxPoints == 16384, "the cap is one below the point area's capacity");
    int wrong = handoff_case(0, 0, 0) + handoff_case(1, 0, 1) + handoff_case(kHandoffMaxPoints, 0, kHandoffMaxPoints) +
                handoff_case(kPairMaxPoints, 0, -1) + handoff_case(5, -1, -1);
    // count words no sender writes, in a heap buffer that ends right behind them: a read past the count is the address sanitizer's report
    for (int count : {kPairMaxPoints, INT_MAX, -2}) {
        std::unique_ptr<float[]> two(new float[2]);
        memcpy(&two[0], &count, 4); two[1] = 0.f;
        int n2 = 0;
        std::vector<float> got(4, 1.f);
        unpack_handoff(two.get(), &n2, got);
        wrong += n2 != -1 || !got.empty();
    }
    printf("%-64s 8 cases, %d wrong\n", "hand-off: 0, 1, cap, cap + 1, failed, foreign counts", wrong);
    return wrong;
}

int main() {
    int bad = 0;
    signal(SIGALRM, hung);
    bad += guard_rounds(4000);
    bad += guard_bound();
    for (int n : {2, 3, 4, 8}) {
        char name[4][80];
        snprintf(name[0], 80, "hub: %d threads, six phases", n);
        snprintf(name[1], 80, "hub: %d threads, one aborts before the first phase", n);
        snprintf(name[2], 80, "hub: %d threads, one aborts between phases", n);
        snprintf(name[3], 80, "hub: %d threads, one aborts inside a broadcast", n);
        const AbortAt at[4] = {kNever, kBefore, kBetween, kInside};
        for (int a = 0; a < 4; ++a) bad += hub_rounds(name[a], n, 500, at[a]);
    }
    bad += roles_table();
    bad += handoff();
    alarm(0);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
