// rccl_comm.cpp — the multi-GPU half of the C ABI (include/poppy_hip.h, "multi-GPU"), its RCCL part: the loader, a context's
// communicator (rccl_comm.h) and the pair state's way between GPUs.
//
// The path shards two ways, and neither needs a collective on the data path:
//   frames of ONE pair   phase-mode frames are independent (src/poppy.hpp:186-200,234-235): every GPU renders a contiguous
//                        sub-range of t_j = j / total.  The only exchange is the pair state — both images, the mask field's
//                        grey complement and the point sets, ONE contiguous allocation (context.h: arena) — which goes from
//                        the GPU that ran the pair set-up to all others in a single ncclBroadcast over RCCL / xGMI.
//   pairs                the pairs loop of the CLI (src/poppy.cpp:266-328) has no cross-pair state: every GPU takes whole
//                        pairs off a shared counter, each a chained sequence on its own context.  No communication at all.
// Two deployment shapes are served by the same primitives:
//   one process per GPU  (bench.py under torch.distributed.run): poppy_hip_comm_id on one rank, the 128 bytes reach the others
//                        by any out-of-band channel, poppy_hip_comm_init everywhere, poppy_hip_pair_broadcast per pair;
//   one process, N GPUs  (a drop-in behind the reference's single-process CLI): poppy_hip_morph_sharded (morph_sharded.cpp) and
//                        poppy_hip_morph_pairs (pool.cpp) run one host thread and one context per device; the former creates
//                        its communicators with ncclCommInitAll.
// librccl is loaded on first use (dlopen): single-GPU callers never touch it, and all entry points come from ONE handle, so a
// second copy of RCCL in the process (PyTorch ships its own) cannot be mixed in by symbol interposition.
#include "rccl_comm.h"
#include <dlfcn.h>

namespace {

struct Id128 { char b[128]; };                  // ncclUniqueId: 128 opaque bytes, passed BY VALUE to ncclCommInitRank
struct Rccl {
    void* handle = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id128, int) = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;      // optional: what the communicator itself says its size is (poppy_hip_comm_info)
    int (*CommUserRank)(void*, int*) = nullptr;
    int (*CommAbort)(void*) = nullptr;            // optional: unblocks the other device threads of poppy_hip_morph_sharded when one of them failed
    int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string err;
};
constexpr int kNcclUint8 = 1, kNcclFloat64 = 8, kNcclMax = 2;       // rccl.h: ncclUint8, ncclFloat64 (ncclDouble), ncclMax

Rccl* rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, []() {
        const char* names[] = {getenv("POPPY_HIP_RCCL"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names) {
            if (!n) continue;
            r.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (r.handle) break;
        }
        if (!r.handle) { r.err = std::string("librccl not found: ") + (dlerror() ? dlerror() : ""); return; }
        auto sym = [&](const char* s) { void* p = dlsym(r.handle, s); if (!p && r.err.empty()) r.err = std::string("librccl lacks ") + s; return p; };
        r.GetUniqueId = (int (*)(void*))sym("ncclGetUniqueId");
        r.CommInitRank = (int (*)(void**, int, Id128, int))sym("ncclCommInitRank");
        r.CommInitAll = (int (*)(void**, int, const int*))sym("ncclCommInitAll");
        r.CommDestroy = (int (*)(void*))sym("ncclCommDestroy");
        r.CommAbort = (int (*)(void*))dlsym(r.handle, "ncclCommAbort");
        r.CommCount = (int (*)(void*, int*))dlsym(r.handle, "ncclCommCount");
        r.CommUserRank = (int (*)(void*, int*))dlsym(r.handle, "ncclCommUserRank");
        r.Broadcast = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))sym("ncclBroadcast");
        r.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))sym("ncclAllReduce");
        r.GetErrorString = (const char* (*)(int))sym("ncclGetErrorString");
    });
    return &r;
}

std::string rccl_error(const char* what, int code) {
    Rccl* r = rccl();
    return std::string(what) + ": " + (r->GetErrorString ? r->GetErrorString(code) : "RCCL error");
}
int rccl_fail(poppy_hip_ctx* c, const char* what, int code) { c->err = rccl_error(what, code); return POPPY_E_DEVICE; }

int no_comm(poppy_hip_ctx* c) {
    return fail(c, POPPY_E_STATE, c->comm.aborted() ? "the communicator was aborted" : "no communicator (poppy_hip_comm_init)");
}

// the small reductions' scratch, with the communicator, where a failure is this rank's alone: inside a collective sequence an allocation that
// fails would leave the other ranks waiting in the reduction this rank never enters
bool alloc_comm_scratch(poppy_hip_ctx* c) {
    return c->d_comm_scratch || hipMalloc((void**)&c->d_comm_scratch, 8 * sizeof(double)) == hipSuccess;
}

}  // namespace

int comm_require(poppy_hip_ctx* c) { return c->comm.present() ? POPPY_OK : no_comm(c); }

int comm_broadcast(poppy_hip_ctx* c, void* d_buf, size_t bytes, int root) {
    {
        CommUse use(c->comm);
        if (!use.comm) return no_comm(c);
        const int nr = rccl()->Broadcast(d_buf, d_buf, bytes, kNcclUint8, root, use.comm, c->stream);
        if (nr != 0) return rccl_fail(c, "ncclBroadcast", nr);
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, POPPY_E_DEVICE, "broadcast");
    return POPPY_OK;
}

// (step timing, the set-up's detail values and status flags; the device scratch is allocated once per context: hipMalloc / hipFree per call
// cost more than the reduction)
int comm_max_n(poppy_hip_ctx* c, double* values, int n) {
    if (n < 1 || n > 8) return fail(c, POPPY_E_ARG, "comm_max_n: 1..8 values");
    if (!c->d_comm_scratch) return fail(c, POPPY_E_STATE, "communicator without its scratch (poppy_hip_comm_init allocates it)");
    double* d = c->d_comm_scratch;
    { const int rc = comm_require(c); if (rc) return rc; }           // (nobody is waiting for this rank in an aborted job: out before the device is touched)
    // nothing below returns before the collective has been entered: a rank whose device selection or copy-in failed still takes part (and
    // returns its error afterwards), so that no rank is left alone inside ncclAllReduce
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = hipMemcpyAsync(d, values, (size_t)n * 8, hipMemcpyHostToDevice, c->stream);
    int nr;
    {
        CommUse use(c->comm);
        if (!use.comm) { (void)hipStreamSynchronize(c->stream); return no_comm(c); }      // (aborted since the check above; the copy-in reads the caller's `values`, and no collective is on the stream)
        nr = rccl()->AllReduce(d, d, (size_t)n, kNcclFloat64, kNcclMax, use.comm, c->stream);   // entered whatever `e` says: see above
    }
    if (e == hipSuccess && nr == 0) e = hipMemcpyAsync(values, d, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (nr != 0) return rccl_fail(c, "ncclAllReduce", nr);
    if (e != hipSuccess) { c->err = std::string("comm_max: ") + hipGetErrorString(e); return POPPY_E_DEVICE; }
    return POPPY_OK;
}

bool comm_abort(poppy_hip_ctx* c) {
    Rccl* r = rccl();
    if (!r->CommAbort) return true;                                  // (a librccl without it: the communicator stays as it is)
    bool drained = true;
    void* cm = c->comm.take_for_abort(&drained);
    if (cm) (void)r->CommAbort(cm);
    return drained;
}

int comm_init_all(poppy_hip_ctx* const* ctxs, const int* devices, int n, std::string* err) {
    Rccl* r = rccl();
    if (!r->err.empty()) { *err = r->err; return POPPY_E_UNSUPPORTED; }
    std::vector<void*> comms(n, nullptr);
    const int rc = r->CommInitAll(comms.data(), n, devices);
    if (rc != 0) { *err = rccl_error("ncclCommInitAll", rc); return POPPY_E_DEVICE; }
    for (int k = 0; k < n; ++k) { ctxs[k]->comm.set(comms[k]); ctxs[k]->comm_rank = k; ctxs[k]->comm_world = n; }
    for (int k = 0; k < n; ++k)                           // before any thread can be inside a collective
        if (hipSetDevice(devices[k]) != hipSuccess || !alloc_comm_scratch(ctxs[k])) { *err = "allocation of the reduction scratch"; return POPPY_E_DEVICE; }
    return POPPY_OK;
}

extern "C" {

int poppy_hip_comm_id(uint8_t* id128) {
    if (!id128) return POPPY_E_ARG;
    Rccl* r = rccl();
    if (!r->err.empty()) return POPPY_E_UNSUPPORTED;
    return r->GetUniqueId(id128) == 0 ? POPPY_OK : POPPY_E_DEVICE;
}

int poppy_hip_comm_init(poppy_hip_ctx* c, int rank, int world, const uint8_t* id128) {
    if (!c) return POPPY_E_ARG;
    if (!id128 || world < 1 || rank < 0 || rank >= world) return fail(c, POPPY_E_ARG, "bad rank / world / id");
    Rccl* r = rccl();
    if (!r->err.empty()) return fail(c, POPPY_E_UNSUPPORTED, r->err.c_str());
    if (c->comm.present() || c->comm.aborted()) return fail(c, POPPY_E_STATE, "this context already has a communicator (poppy_hip_comm_free first)");
    HIPCHK(c, hipSetDevice(c->device));
    Id128 id;
    memcpy(id.b, id128, 128);
    void* comm = nullptr;
    const int rc = r->CommInitRank(&comm, world, id, rank);
    if (rc != 0) return rccl_fail(c, "ncclCommInitRank", rc);
    if (!alloc_comm_scratch(c)) {
        (void)r->CommDestroy(comm);
        return fail(c, POPPY_E_DEVICE, "allocation of the reduction scratch");
    }
    c->comm.set(comm); c->comm_rank = rank; c->comm_world = world;
    return POPPY_OK;
}

// what the context believes (rank, world) and what its RCCL communicator reports (ncclCommUserRank, ncclCommCount; -1: no communicator / symbol missing)
int poppy_hip_comm_info(poppy_hip_ctx* c, int* rank, int* world, int* nccl_rank, int* nccl_count) {
    if (!c) return POPPY_E_ARG;
    if (rank) *rank = c->comm_rank;
    if (world) *world = c->comm_world;
    int nr = -1, nc = -1;
    Rccl* r = rccl();
    CommUse use(c->comm);
    if (use.comm && r->handle) {
        if (r->CommUserRank && r->CommUserRank(use.comm, &nr) != 0) nr = -1;
        if (r->CommCount && r->CommCount(use.comm, &nc) != 0) nc = -1;
    }
    if (nccl_rank) *nccl_rank = nr;
    if (nccl_count) *nccl_count = nc;
    return POPPY_OK;
}

int poppy_hip_comm_free(poppy_hip_ctx* c) {
    if (!c) return POPPY_E_ARG;
    void* cm = c->comm.take();                                      // (an aborted communicator is gone already: its pointer was taken by the abort)
    if (cm) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        (void)rccl()->CommDestroy(cm);
    }
    c->comm.clear_aborted(); c->comm_rank = 0; c->comm_world = 1;
    return POPPY_OK;
}

int poppy_hip_comm_max(poppy_hip_ctx* c, double* value) {
    if (!c || !value) return POPPY_E_ARG;
    const int rc = comm_require(c);
    return rc ? rc : comm_max_n(c, value, 1);
}

int poppy_hip_pair_state_bytes(int width, int height, size_t* bytes) {
    if (width <= 0 || height <= 0 || !bytes) return POPPY_E_ARG;
    *bytes = pair_state_bytes(width, height);
    return POPPY_OK;
}

// The resident pair of rank `root` becomes the resident pair of every rank: one ncclBroadcast of the packed pair state.
// Everything that can fail on ONE rank (the root's pair missing or holding more points than the state has room for, an allocation on
// a receiver) happens first, and the ranks then agree on the outcome through a one-value reduction: a rank never returns with an
// error while the others are already blocked inside the broadcast.
int poppy_hip_pair_broadcast(poppy_hip_ctx* c, int root, int W, int H) {
    if (!c) return POPPY_E_ARG;
    int rc = comm_require(c); if (rc) return rc;
    if (root < 0 || root >= c->comm_world || W <= 0 || H <= 0) return fail(c, POPPY_E_ARG, "bad root / geometry");   // the same on every rank
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    if (c->comm_rank == root) {
        if (!c->pair_ready || c->W != W || c->H != H) rc = fail(c, POPPY_E_STATE, "the root has no resident pair of this geometry");
        else rc = stage_pair_state(c);
    } else {
        rc = alloc_pair(c, W, H);
        if (rc == POPPY_OK) c->pair_ready = false;
    }
    if (c->comm_world > 1) {
        double worst = rc == POPPY_OK ? 0.0 : 1.0;
        const int ra = comm_max_n(c, &worst, 1);                   // a collective: entered by every rank whatever its own outcome
        if (ra != POPPY_OK) return ra;
        if (rc != POPPY_OK) return rc;
        if (worst != 0.0) return fail(c, POPPY_E_STATE, "another rank could not take part in the broadcast (its own error says why)");
    } else if (rc != POPPY_OK) return rc;
    rc = comm_broadcast(c, c->arena, c->arena_bytes, root); if (rc) return rc;
    return c->comm_rank != root ? adopt_pair_state(c) : POPPY_OK;
}

// The packed pair state to / from a caller's device buffer (one device copy): for callers that move it with their own
// transport (bench.py falls back to torch.distributed when librccl cannot be initialised a second time in the process).
int poppy_hip_pair_export_device(poppy_hip_ctx* c, void* d_dst, size_t bytes) {
    if (!c || !d_dst) return POPPY_E_ARG;
    if (!c->pair_ready) return fail(c, POPPY_E_STATE, "no resident pair");
    if (bytes < c->arena_bytes) return fail(c, POPPY_E_ARG, "buffer smaller than poppy_hip_pair_state_bytes");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = stage_pair_state(c); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(d_dst, c->arena, c->arena_bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return POPPY_OK;
}
int poppy_hip_pair_import_device(poppy_hip_ctx* c, const void* d_src, size_t bytes, int W, int H) {
    if (!c || !d_src || W <= 0 || H <= 0) return POPPY_E_ARG;
    if (bytes < pair_state_bytes(W, H)) return fail(c, POPPY_E_ARG, "buffer smaller than poppy_hip_pair_state_bytes");
    HIPCHK(c, hipSetDevice(c->device));
    chain_touch(c);
    int rc = alloc_pair(c, W, H); if (rc) return rc;
    c->pair_ready = false;
    HIPCHK(c, hipMemcpyAsync(c->arena, d_src, c->arena_bytes, hipMemcpyDeviceToDevice, c->stream));
    return adopt_pair_state(c);
}

}  // extern "C"
