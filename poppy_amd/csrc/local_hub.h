// local_hub.h — the in-process transport of the sharded pair set-up (sharded_setup.cpp): n contexts of one process, one host thread each,
// exchange through a barrier instead of RCCL.  Nothing of HIP in here (the device copy of a broadcast is the caller's):
// tools/comm_guard_check.cpp runs the hub alone under the thread and address sanitizers.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <mutex>

namespace poppy_hip {

struct LocalHub {
    static constexpr int kMaxValues = 8;                  // as the RCCL reduction (rccl_comm.h: comm_max_n)
    explicit LocalHub(int n_) : n(n_) {}
    // A context left the protocol with an error: whoever waits here, now or later, returns false instead of waiting for ever.
    void abort() { { std::lock_guard<std::mutex> g(mu); aborted = true; } cv.notify_all(); }

    // Broadcast of one buffer: the root publishes where its buffer lies, every other thread runs copy_from(root's buffer, root's device)
    // between two barriers — the root's buffer may change again only behind the second.  false: the hub was aborted (copy_from may not have run).
    template <class Copy>
    bool broadcast_slot(bool is_root, const void* buf, int device, Copy&& copy_from) {
        if (is_root) { std::lock_guard<std::mutex> g(mu); src = buf; src_device = device; }
        if (!barrier()) return false;
        if (!is_root) copy_from(src, src_device);          // (written before the barrier, read behind it)
        return barrier();
    }
    // v[0..m) becomes the maximum over all threads, m <= kMaxValues.  false: the hub was aborted (v is unchanged).
    bool all_max(int rank, double* v, int m) {
        m = std::min(m, (int)kMaxValues);
        if (!barrier()) return false;                      // nobody still reads the previous reduction's values
        if (rank == 0) std::fill(vals, vals + kMaxValues, -1e300);
        if (!barrier()) return false;
        { std::lock_guard<std::mutex> g(mu); for (int i = 0; i < m; ++i) vals[i] = std::max(vals[i], v[i]); }
        if (!barrier()) return false;
        for (int i = 0; i < m; ++i) v[i] = vals[i];
        return true;
    }

private:
    bool barrier() {
        std::unique_lock<std::mutex> g(mu);
        if (aborted) return false;
        const unsigned ph = phase;
        if (++arrived == n) { arrived = 0; ++phase; cv.notify_all(); return true; }
        cv.wait(g, [&] { return phase != ph || aborted; });
        return phase != ph;                                // a phase that every thread reached stays complete: an abort raised behind it is the next barrier's to report
    }
    const int n;
    std::mutex mu; std::condition_variable cv; int arrived = 0; unsigned phase = 0;
    const void* src = nullptr; int src_device = 0;
    double vals[kMaxValues] = {};
    bool aborted = false;
};

}  // namespace poppy_hip
