// rccl_comm.h — a context's RCCL communicator as the other units see it (rccl_comm.cpp): whether there is one, the two collectives that
// everything on it goes through, and the abort.  Nobody else reads poppy_hip_ctx::comm or calls into librccl.
#pragma once
#include "context.h"

// POPPY_OK, or POPPY_E_STATE with the reason in c->err: no communicator yet, or the communicator was aborted
int comm_require(poppy_hip_ctx* c);
// The two collectives, complete on return.  Each enqueues under a CommUse (comm_guard.h) and waits for c->stream outside it: a rank blocked in
// that wait is what the abort exists to unblock.  An aborted communicator: POPPY_E_STATE (nobody is waiting for this rank in an aborted job).
int comm_broadcast(poppy_hip_ctx* c, void* d_buf, size_t bytes, int root);           // in place, device memory
int comm_max_n(poppy_hip_ctx* c, double* values, int n);                             // max over the ranks of n <= 8 host doubles
// Takes the communicator out of the context and ncclCommAbort's it (which frees it): pending and later collectives of every rank fail instead of
// waiting.  false: a thread was still handing the pointer to RCCL when kCommAbortBoundMs had passed, and the abort went ahead regardless.
bool comm_abort(poppy_hip_ctx* c);
// One communicator (rank k of n) and its reduction scratch for each of n fresh contexts on devices[k], for one process that drives them all.
// On failure *err says why and the caller frees whatever the contexts got (poppy_hip_comm_free).
int comm_init_all(poppy_hip_ctx* const* ctxs, const int* devices, int n, std::string* err);
