// The host runtime's call API (not part of the ABI): what a compute call of
// any subsystem uses of a context -- the planners, the SMO and AUC-gradient
// hosts beside their kernels, the sharded Gram.  Defined in host/context.cpp
// (comm_destroy: host/shard.cpp); the structs behind the
// handles are in host/runtime_types.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

struct sk_context;
struct sk_dataset;

namespace sk {
// accessors into the context
hipStream_t ctx_stream(sk_context* ctx);
int ctx_device(sk_context* ctx);
void*& ctx_comm(sk_context* ctx);
int ctx_fail(sk_context* ctx, int code, const std::string& msg);
void comm_destroy(void* comm);
// a compute call's timing set, launch events and uploads
hipError_t lev_mark(sk_context* ctx, hipStream_t s);
hipError_t lev_collect(sk_context* ctx);
void lev_reset(sk_context* ctx);
hipError_t tset_resolve(sk_context* ctx, int k);
hipError_t call_begin(sk_context* ctx);
hipError_t call_finish(sk_context* ctx, hipStream_t s, bool stem, bool str);
hipError_t h2d(sk_context* ctx, void* dst, const void* src, size_t bytes, hipStream_t s);
hipError_t up_reserve(sk_context* ctx, size_t bytes, char** dst);
hipError_t up_copy(sk_context* ctx, const void* src, size_t bytes, hipStream_t s);
// the context's reusable device buffers; a dataset uploaded to its device
int ensure_work(sk_context* ctx, size_t bytes);
int ensure_scratch(sk_context* ctx, size_t bytes);
int check_set(sk_context* ctx, sk_dataset* ds);
}  // namespace sk
