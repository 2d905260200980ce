// writer_buffers.h — the two ways the writer path owns device memory.  Nothing of the context in here: tools/writer_buffers_check.cpp runs both types alone,
// against a stub allocator, under the address sanitizer.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <vector>

// A buffer that lives as long as its context and only grows: the scratch of the frames that no slot renders, the sequence's store and rings.
struct DeviceBuffer {
    uint8_t* p = nullptr;
    size_t bytes = 0;
    // at least `need` bytes; the contents do not survive growth.  sync_first: a stream whose queued work may still read the buffer that growth frees.
    // A failure leaves the buffer empty (a failed synchronise: as it was).
    hipError_t reserve(size_t need, hipStream_t sync_first = nullptr) {
        if (need <= bytes) return hipSuccess;
        if (sync_first) { const hipError_t e = hipStreamSynchronize(sync_first); if (e != hipSuccess) return e; }
        release();
        const hipError_t e = hipMalloc((void**)&p, need);
        if (e != hipSuccess) p = nullptr; else bytes = need;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

// The device buffers of one call, freed when the call leaves, whichever way.  The caller synchronises its stream first: nothing of the call is in flight when they go.
struct CallBuffers {
    std::vector<void*> held;
    CallBuffers() = default;
    CallBuffers(const CallBuffers&) = delete;
    CallBuffers& operator=(const CallBuffers&) = delete;
    ~CallBuffers() { for (void* b : held) (void)hipFree(b); }
    hipError_t alloc(uint8_t** p, size_t bytes) {                  // *p: the buffer, null behind a failure
        const hipError_t e = hipMalloc((void**)p, bytes);
        if (e != hipSuccess) *p = nullptr; else held.push_back(*p);
        return e;
    }
};
