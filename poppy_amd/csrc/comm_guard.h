// comm_guard.h — who may hand a context's RCCL communicator to RCCL, and when the abort path may free it (rccl_comm.cpp holds the only users).
// Nothing of HIP or RCCL in here: tools/comm_guard_check.cpp runs the type alone, user threads against an aborter that really frees the
// object, under the thread and address sanitizers.
#pragma once
#include <atomic>
#include <chrono>
#include <thread>

namespace poppy_hip {

// How long take_for_abort waits for the threads that are inside an enter() / leave() bracket.  The bracket spans RCCL's ENQUEUE call alone
// (ncclBroadcast / ncclAllReduce return once the operation is on the stream; they do not wait for the other ranks — the wait is the stream
// synchronise, outside the bracket), so it is microseconds long and the bound can be short.  Its value is a guess all the same: an abort
// needs two or more devices, so it cannot be measured on one GPU.
#ifndef POPPY_COMM_ABORT_BOUND_MS
#define POPPY_COMM_ABORT_BOUND_MS 200
#endif
constexpr int kCommAbortBoundMs = POPPY_COMM_ABORT_BOUND_MS;

// The communicator pointer, a count of the threads that are handing it to RCCL right now, and the "was aborted" flag.
// Every operation is sequentially consistent.  A user increments the count and THEN loads the pointer; the aborter exchanges the pointer to
// null and THEN reads the count: either the user sees null, or the aborter sees the user and waits for its leave().  So a pointer that
// take_for_abort returns with *drained == true is in nobody's hands.  With *drained == false — a user sat in its bracket for longer than
// the bound — that user may still be inside RCCL with the pointer: the caller aborts all the same (a job that has failed must not wait for
// ever), which is what the code did for every user before this guard existed.
class CommHandle {
public:
    void* enter() {                                       // null: no communicator (none yet, freed, or aborted) — and then no leave()
        users_.fetch_add(1);
        void* p = ptr_.load();
        if (!p) users_.fetch_sub(1);
        return p;
    }
    void leave() { users_.fetch_sub(1); }
    bool present() const { return ptr_.load() != nullptr; }
    void set(void* p) { ptr_.store(p); }
    void* take() { return ptr_.exchange(nullptr); }       // for comm_free, on the owner's thread: no collective of this context is in flight
    void* take_for_abort(bool* drained) {
        aborted_.store(true);
        void* p = ptr_.exchange(nullptr);
        const auto until = std::chrono::steady_clock::now() + std::chrono::milliseconds(kCommAbortBoundMs);
        // (one reading of zero is enough, and it is the one that counts: whoever enters from here on finds null, and only bumps the count on its way out)
        while (!(*drained = users_.load() == 0) && std::chrono::steady_clock::now() < until) std::this_thread::yield();
        return p;
    }
    bool aborted() const { return aborted_.load(); }      // since the last clear_aborted: the context takes no new communicator until then
    void clear_aborted() { aborted_.store(false); }

private:
    std::atomic<void*> ptr_{nullptr};
    std::atomic<int> users_{0};
    std::atomic<bool> aborted_{false};
};

// One enter() / leave() bracket.  comm == null: there is no communicator to use.
struct CommUse {
    CommHandle& h; void* const comm;
    explicit CommUse(CommHandle& h_) : h(h_), comm(h_.enter()) {}
    ~CommUse() { if (comm) h.leave(); }
    CommUse(const CommUse&) = delete;
    CommUse& operator=(const CommUse&) = delete;
};

}  // namespace poppy_hip
