// setup_latch.h — what the two chain threads of a pair set-up (pair_begin.cpp) wait for each other with.  Nothing of HIP in here:
// tools/setup_latch_check.cpp runs these types alone, two threads over a few thousand rounds, under the thread and address sanitizers.
#pragma once
#include <condition_variable>
#include <mutex>

namespace poppy_hip {

// A counter that threads wait on (no spinning: the wait can be a chain's length).  The set-up counts the images whose dft_detail2 value is
// known — each chain goes on to the detector's second half, which takes nfeatures and so BOTH details (src/extractor.cpp:40-45), once it reads 2.
struct Details {
    void add() { { std::lock_guard<std::mutex> g(m); ++n; } cv.notify_all(); }
    void wait_for(int k) { std::unique_lock<std::mutex> g(m); cv.wait(g, [&] { return n >= k; }); }
private:
    std::mutex m; std::condition_variable cv; int n = 0;
};

// One chain's entry in a Details: counts once, at the detail or at whichever exit comes first (a chain that fails before its detail still counts,
// so the other chain is not left waiting for it).
struct Publish {
    Details& d; bool done = false;
    void now() { if (!done) { done = true; d.add(); } }
    ~Publish() { now(); }
};

// Whether the second host image's upload, queued by the second chain's thread on that chain's stream, has been queued and its event recorded: the
// first chain's thread waits here (host) before it orders gabor2's stream behind that event (device).  known() keeps the first answer given.
struct UploadKnown {
    void pending() { state = 0; }                          // before the threads start: there is a staged upload to wait for
    void known(bool ok) { { std::lock_guard<std::mutex> g(m); if (state) return; state = ok ? 1 : -1; } cv.notify_all(); }
    bool wait() { std::unique_lock<std::mutex> g(m); cv.wait(g, [&] { return state != 0; }); return state > 0; }     // false: the upload failed or never happened
private:
    std::mutex m; std::condition_variable cv; int state = 1;
};
// The uploading chain's exit: the first chain is never left waiting for the second's upload, whichever way the second leaves.
struct UploadExit {
    UploadKnown& u; bool mine;
    ~UploadExit() { if (mine) u.known(false); }
};

}  // namespace poppy_hip
