// writer_buffers_check.cpp — the writer path's two buffer owners (poppy_amd/csrc/writer_buffers.h) alone, on the host, under a sanitizer:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/writer_buffers_check.cpp -o /tmp/buffers_asan && /tmp/buffers_asan
// No HIP runtime is linked: hipMalloc, hipFree and hipStreamSynchronize are the stubs below, malloc and free that count their calls and can be told to fail the
// next allocation or the next synchronise.  A double free, a leak or a use of a freed buffer is the sanitizer's to report; the counts catch what it cannot see.
#include "../poppy_amd/csrc/writer_buffers.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int g_allocs = 0, g_frees = 0, g_syncs = 0;
static bool g_fail_alloc = false, g_fail_sync = false;

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_fail_alloc) { g_fail_alloc = false; return hipErrorOutOfMemory; }      // (*p stays as it was, as with the runtime)
    *p = malloc(bytes);
    memset(*p, 0xA5, bytes);                                       // every byte of it is the caller's
    ++g_allocs;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) { free(p); ++g_frees; return hipSuccess; }
extern "C" hipError_t hipStreamSynchronize(hipStream_t) {
    ++g_syncs;
    if (g_fail_sync) { g_fail_sync = false; return hipErrorUnknown; }
    return hipSuccess;
}

static int bad = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++bad; } } while (0)

static hipStream_t const kStream = (hipStream_t)(uintptr_t)0x40;   // never dereferenced: the stub only counts

static void grow_only() {
    DeviceBuffer b;
    CHECK(b.reserve(0) == hipSuccess && !b.p && b.bytes == 0 && g_allocs == 0);      // nothing needed, nothing allocated
    CHECK(b.reserve(100) == hipSuccess && b.p && b.bytes == 100 && g_allocs == 1 && g_frees == 0);
    memset(b.p, 1, 100);
    uint8_t* first = b.p;
    CHECK(b.reserve(40, kStream) == hipSuccess && b.p == first && b.bytes == 100);   // smaller: as it is, and no synchronise for it
    CHECK(b.reserve(100, kStream) == hipSuccess && b.p == first && g_syncs == 0);    // equal: likewise
    CHECK(b.reserve(101) == hipSuccess && b.bytes == 101 && g_allocs == 2 && g_frees == 1 && g_syncs == 0);      // larger, no stream: freed and allocated, not synchronised
    memset(b.p, 2, 101);
    CHECK(b.reserve(4096, kStream) == hipSuccess && b.bytes == 4096 && g_allocs == 3 && g_frees == 2 && g_syncs == 1);      // ... with one: synchronised first
    memset(b.p, 3, 4096);
    g_fail_sync = true;                                            // the synchronise fails: the buffer stays as it was
    first = b.p;
    CHECK(b.reserve(8192, kStream) == hipErrorUnknown && b.p == first && b.bytes == 4096 && g_frees == 2);
    g_fail_alloc = true;                                           // the allocation fails: empty, the old buffer freed once
    CHECK(b.reserve(8192) == hipErrorOutOfMemory && !b.p && b.bytes == 0 && g_allocs == 3 && g_frees == 3);
    b.release();                                                   // ... and not a second time
    CHECK(g_frees == 3);
    CHECK(b.reserve(16) == hipSuccess && b.p && b.bytes == 16 && g_allocs == 4);     // an empty buffer grows again
    b.release();
    b.release();                                                   // twice
    CHECK(!b.p && b.bytes == 0 && g_frees == 4);
}

static int leaves_early(bool early) {
    CallBuffers held;
    uint8_t *a = nullptr, *b = nullptr;
    if (held.alloc(&a, 64) != hipSuccess || held.alloc(&b, 32) != hipSuccess) return -1;
    memset(a, 4, 64); memset(b, 5, 32);
    if (early) return 1;
    return 0;
}

static void call_scoped() {
    const int allocs = g_allocs, frees = g_frees;
    CHECK(leaves_early(true) == 1 && g_allocs == allocs + 2 && g_frees == frees + 2);      // an early return frees both
    CHECK(leaves_early(false) == 0 && g_allocs == allocs + 4 && g_frees == frees + 4);
    g_fail_alloc = true;                                           // the first allocation fails: nothing held, nothing freed
    CHECK(leaves_early(false) == -1 && g_allocs == allocs + 4 && g_frees == frees + 4);
    {
        CallBuffers held;
        uint8_t *a = nullptr, *b = (uint8_t*)(uintptr_t)1;
        CHECK(held.alloc(&a, 8) == hipSuccess);
        g_fail_alloc = true;                                       // a failure behind a success: a null pointer, the first still held
        CHECK(held.alloc(&b, 8) == hipErrorOutOfMemory && !b && held.held.size() == 1);
    }
    CHECK(g_allocs - g_frees == allocs - frees);                   // every buffer of every holder has gone, once
}

int main() {
    grow_only();
    call_scoped();
    CHECK(g_allocs == g_frees);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
