// The context behind sk_context: a compute call's timing sets (a ring when
// asynchronous), launch events and uploads (host/runtime.h), the reusable
// device buffers, and the entry points that open, close and inspect a context.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>

#include "host/feature_gram.h"
#include "host/runtime_types.h"

namespace sk {
hipStream_t ctx_stream(sk_context* ctx) { return ctx->stream; }

// start or end event of one dominant-kernel launch, on the launch's stream
hipError_t lev_mark(sk_context* ctx, hipStream_t s) {
  sk_context::TSet& T = ctx->tset[ctx->tk];
  if (T.lev_used == T.lev.size()) {
    hipEvent_t e = nullptr;
    const hipError_t r = hipEventCreate(&e);
    if (r != hipSuccess) return r;
    T.lev.push_back(e);
  }
  return hipEventRecord(T.lev[T.lev_used++], s);
}

// after the launch streams are synchronized: adds the marked launches'
// durations to the call's sum
hipError_t lev_collect(sk_context* ctx) {
  sk_context::TSet& T = ctx->tset[ctx->tk];
  for (size_t i = 0; i + 1 < T.lev_used; i += 2) {
    float ms = 0.f;
    const hipError_t r = hipEventElapsedTime(&ms, T.lev[i], T.lev[i + 1]);
    if (r != hipSuccess) return r;
    ctx->last_launch_ms_sum += ms;
    ++ctx->last_launch_n;
  }
  T.lev_used = 0;
  return hipSuccess;
}

// A pending asynchronous call's timing, into the acc_* totals (waits for it).
hipError_t tset_resolve(sk_context* ctx, int k) {
  sk_context::TSet& T = ctx->tset[k];
  if (!T.pending) return hipSuccess;
  T.pending = false;
  float ms = 0.f;
  hipError_t r;
  if (T.stem) {
    if ((r = hipEventSynchronize(T.ev[1])) != hipSuccess) return r;
    if ((r = hipEventElapsedTime(&ms, T.ev[0], T.ev[1])) != hipSuccess) return r;
    ctx->acc_stem_ms += ms;
  }
  if (T.str) {
    if ((r = hipEventSynchronize(T.ev[3])) != hipSuccess) return r;
    if ((r = hipEventElapsedTime(&ms, T.ev[2], T.ev[3])) != hipSuccess) return r;
    ctx->acc_str_ms += ms;
  }
  for (size_t i = 0; i + 1 < T.lev_used; i += 2) {
    if ((r = hipEventSynchronize(T.lev[i + 1])) != hipSuccess) return r;
    if ((r = hipEventElapsedTime(&ms, T.lev[i], T.lev[i + 1])) != hipSuccess) return r;
    ctx->acc_launch_ms += ms;
    ++ctx->acc_launch_n;
  }
  T.lev_used = 0;
  ctx->acc_cells += T.cells;
  ctx->acc_launches += T.launches;
  return hipSuccess;
}

// Start of a compute call: its timing set (and, async, its staging slot).
hipError_t call_begin(sk_context* ctx) {
  hipError_t r;
  if (ctx->async) {
    const int k = (ctx->tk + 1) % sk_context::kTSets;
    if ((r = tset_resolve(ctx, k)) != hipSuccess) return r;  // the ring came round
    ctx->tk = k;
    sk_context::Stage& G = ctx->stage[ctx->ncalls++ & 1];
    if (G.recorded) {
      if ((r = hipEventSynchronize(G.ev)) != hipSuccess) return r;
    } else if (G.blk || G.off) {
      // the slot's call staged copies but failed before call_finish recorded
      // its event: the copy engine may still read the pinned bytes
      if ((r = hipStreamSynchronize(ctx->stream)) != hipSuccess) return r;
      if (ctx->cps && (r = hipStreamSynchronize(ctx->cps)) != hipSuccess) return r;
    }
    G.recorded = false;
    G.blk = G.off = 0;
  } else {
    ctx->tk = 0;
  }
  sk_context::TSet& T = ctx->tset[ctx->tk];
  for (int i = 0; i < 4; ++i)
    if (!T.ev[i] && (r = hipEventCreate(&T.ev[i])) != hipSuccess) return r;
  T.lev_used = 0;
  T.pending = false;
  ctx->ev0 = T.ev[0];
  ctx->ev1 = T.ev[1];
  ctx->ev2 = T.ev[2];
  ctx->ev3 = T.ev[3];
  return hipSuccess;
}

// Host-to-device upload of a compute call: straight from the caller's memory
// (synchronous calls), or through the call's pinned staging slot (async).
hipError_t h2d(sk_context* ctx, void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (bytes == 0) return hipSuccess;
  if (!ctx->async) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
  sk_context::Stage& G = ctx->stage[(ctx->ncalls - 1) & 1];
  const size_t need = (bytes + 255) & ~(size_t)255;
  while (G.blk < G.blocks.size() && G.off + need > G.blocks[G.blk].second) {
    ++G.blk;
    G.off = 0;
  }
  if (G.blk == G.blocks.size()) {
    const size_t cap = std::max(need, (size_t)8 << 20);
    void* p = nullptr;
    const hipError_t r = hipHostMalloc(&p, cap, hipHostMallocDefault);
    if (r != hipSuccess) return r;
    G.blocks.push_back({static_cast<char*>(p), cap});
    G.off = 0;
  }
  char* p = G.blocks[G.blk].first + G.off;
  G.off += need;
  std::memcpy(p, src, bytes);
  return hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s);
}

// Asynchronous calls (BPLA): the call's host inputs go to a device buffer of
// the call's parity on a copy stream that the call's stream then waits for,
// so the upload overlaps the previous call's kernels instead of following
// them.  The buffer's last user is the call two back, which call_begin has
// waited for.
hipError_t up_reserve(sk_context* ctx, size_t bytes, char** dst) {
  sk_context::Stage& G = ctx->stage[(ctx->ncalls - 1) & 1];
  hipError_t r;
  if (G.dcap < bytes) {
    if (G.dbuf && (r = hipFree(G.dbuf)) != hipSuccess) return r;
    G.dbuf = nullptr;
    G.dcap = 0;
    const size_t cap = bytes + bytes / 4 + 4096;
    void* p = nullptr;
    if ((r = hipMalloc(&p, cap)) != hipSuccess) return r;
    G.dbuf = static_cast<char*>(p);
    G.dcap = cap;
  }
  *dst = G.dbuf;
  return hipSuccess;
}

hipError_t up_copy(sk_context* ctx, const void* src, size_t bytes, hipStream_t s) {
  sk_context::Stage& G = ctx->stage[(ctx->ncalls - 1) & 1];
  hipError_t r;
  if (!ctx->cps && (r = hipStreamCreateWithFlags(&ctx->cps, hipStreamNonBlocking)) != hipSuccess) return r;
  if (!G.uev && (r = hipEventCreateWithFlags(&G.uev, hipEventDisableTiming)) != hipSuccess) return r;
  if ((r = h2d(ctx, G.dbuf, src, bytes, ctx->cps)) != hipSuccess) return r;  // (pinned staging)
  if ((r = hipEventRecord(G.uev, ctx->cps)) != hipSuccess) return r;
  return hipStreamWaitEvent(s, G.uev, 0);
}

// End of a compute call whose span events (ev0/ev1: stem, ev2/ev3: string)
// and launch events were recorded on streams joined into `s`: synchronous,
// its timing becomes last_*; async, it stays pending.
hipError_t call_finish(sk_context* ctx, hipStream_t s, bool stem, bool str) {
  sk_context::TSet& T = ctx->tset[ctx->tk];
  T.stem = stem;
  T.str = str;
  T.cells = ctx->last_cells;
  T.launches = ctx->last_launches;
  hipError_t r;
  if (ctx->async) {
    sk_context::Stage& G = ctx->stage[(ctx->ncalls - 1) & 1];
    if ((r = hipEventRecord(G.ev, s)) != hipSuccess) return r;
    G.recorded = true;
    T.pending = true;
    return hipSuccess;
  }
  if ((r = hipStreamSynchronize(s)) != hipSuccess) return r;
  float ms = 0.f;
  if (stem) {
    if ((r = hipEventElapsedTime(&ms, T.ev[0], T.ev[1])) != hipSuccess) return r;
    ctx->last_stem_ms = ms;
  }
  if (str) {
    if ((r = hipEventElapsedTime(&ms, T.ev[2], T.ev[3])) != hipSuccess) return r;
    ctx->last_str_ms = ms;
  }
  return lev_collect(ctx);
}

void lev_reset(sk_context* ctx) {  // (the call's launch events: call_begin)
  ctx->last_launch_ms_sum = 0.0;
  ctx->last_launch_n = 0;
}
int ctx_device(sk_context* ctx) { return ctx->device; }
void*& ctx_comm(sk_context* ctx) { return ctx->comm; }

// ------------------------------------------------------------ work buffers
int ensure_work(sk_context* ctx, size_t bytes) {
  if (ctx->work_bytes >= bytes) return SK_OK;
  if (ctx->work) {
    SK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(ctx->work);
    ctx->work = nullptr;
    ctx->work_bytes = 0;
  }
  const size_t b = std::max(bytes, size_t(1) << 20);
  SK_HIP(ctx, hipMalloc(&ctx->work, b));
  ctx->work_bytes = b;
  return SK_OK;
}

int ensure_scratch(sk_context* ctx, size_t bytes) {
  if (ctx->scratch_bytes >= bytes) return SK_OK;
  if (ctx->scratch) {
    SK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(ctx->scratch);
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
  }
  void* p = nullptr;
  SK_HIP(ctx, hipMalloc(&p, bytes));
  ctx->scratch = static_cast<double*>(p);
  ctx->scratch_bytes = bytes;
  return SK_OK;
}

int check_set(sk_context* ctx, sk_dataset* ds) {
  if (!ds) return fail(ctx, SK_ERR_INVALID, "null dataset");
  if (!ds->uploaded || ds->device != ctx->device)
    return fail(ctx, SK_ERR_INVALID, "dataset not uploaded to this context's device");
  return SK_OK;
}

int ctx_fail(sk_context* ctx, int code, const std::string& msg) { return fail(ctx, code, msg); }

}  // namespace sk

extern "C" {

const char* sk_strerror(int s) {
  switch (s) {
    case SK_OK: return "ok";
    case SK_ERR_INVALID: return "invalid argument";
    case SK_ERR_HIP: return "HIP runtime error";
    case SK_ERR_NO_DEVICE: return "no usable gfx950 device";
    case SK_ERR_ALLOC: return "allocation failed";
    case SK_ERR_RANGE: return "index out of range";
    case SK_ERR_UNSUPPORTED: return "unsupported";
    default: return "unknown status";
  }
}

const char* sk_last_error(const sk_context* ctx) { return ctx ? ctx->err.c_str() : ""; }

int sk_open(int device, void* hip_stream, sk_context** out) {
  if (!out) return SK_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SK_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return SK_ERR_RANGE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SK_ERR_NO_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SK_ERR_NO_DEVICE;
  std::unique_ptr<sk_context> c(new (std::nothrow) sk_context());
  if (!c) return SK_ERR_ALLOC;
  c->device = device;
  c->n_cu = prop.multiProcessorCount;
  if (hipSetDevice(device) != hipSuccess) return SK_ERR_HIP;
  if (hip_stream) {
    c->stream = static_cast<hipStream_t>(hip_stream);
  } else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return SK_ERR_HIP;
    c->own_stream = true;
  }
  // a failure part-way releases what was created (sk_close skips nulls)
  if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->cls, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->eva, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->evf, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->evj, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->evk, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->evx, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->stage[0].ev, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->stage[1].ev, hipEventDisableTiming) != hipSuccess ||
      sk::call_begin(c.get()) != hipSuccess) {  // (creates timing set 0: ev0..ev3)
    sk_close(c.release());
    return SK_ERR_HIP;
  }
  *out = c.release();
  return SK_OK;
}

int sk_close(sk_context* ctx) {
  if (!ctx) return SK_OK;
  (void)hipSetDevice(ctx->device);
  // work may still be queued on any of the context's streams (e.g. after an
  // error part-way through a multi-stream call): drain them all before the
  // buffers they read are freed
  for (hipStream_t st : {ctx->stream, ctx->side, ctx->cls, ctx->aux, ctx->cps})
    if (st) (void)hipStreamSynchronize(st);
  sk::feat_dots_forget(ctx, nullptr);  // the feature-vector Grams' resident dot matrices
  sk::comm_destroy(ctx->comm);
  ctx->comm = nullptr;
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->work) (void)hipFree(ctx->work);
  if (ctx->s4d.pairs) (void)hipFree(ctx->s4d.pairs);
  if (ctx->s4d.items) (void)hipFree(ctx->s4d.items);
  if (ctx->s4d.band) (void)hipFree(ctx->s4d.band);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  if (ctx->cls) (void)hipStreamDestroy(ctx->cls);
  if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
  for (hipEvent_t e : {ctx->evf, ctx->evj, ctx->evk, ctx->evx, ctx->eva})
    if (e) (void)hipEventDestroy(e);
  for (auto& T : ctx->tset) {  // (ev0..ev3 are the current set's)
    for (hipEvent_t e : T.ev)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : T.lev) (void)hipEventDestroy(e);
  }
  for (auto& G : ctx->stage) {
    if (G.ev) (void)hipEventDestroy(G.ev);
    if (G.uev) (void)hipEventDestroy(G.uev);
    if (G.dbuf) (void)hipFree(G.dbuf);
    for (auto& b : G.blocks) (void)hipHostFree(b.first);
  }
  if (ctx->cps) (void)hipStreamDestroy(ctx->cps);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return SK_OK;
}

int sk_last_timing(const sk_context* ctx, double* stem_ms, double* string_ms, double* cells,
                   int32_t* launches) {
  if (!ctx) return SK_ERR_INVALID;
  if (stem_ms) *stem_ms = ctx->last_stem_ms;
  if (string_ms) *string_ms = ctx->last_str_ms;
  if (cells) *cells = ctx->last_cells;
  if (launches) *launches = ctx->last_launches;
  return SK_OK;
}

int sk_set_async(sk_context* ctx, int32_t on) {
  if (!ctx) return SK_ERR_INVALID;
  if (ctx->async && !on) {  // resolve what is pending first
    const int rc = sk_sync_timing(ctx);
    if (rc) return rc;
  }
  ctx->async = on != 0;
  return SK_OK;
}

int sk_sync_timing(sk_context* ctx) {
  if (!ctx) return SK_ERR_INVALID;
  if (!ctx->async) return SK_OK;
  for (int k = 0; k < sk_context::kTSets; ++k)
    if (sk::tset_resolve(ctx, k) != hipSuccess) return sk::fail(ctx, SK_ERR_HIP, "sk_sync_timing: event");
  ctx->last_stem_ms = ctx->acc_stem_ms;
  ctx->last_str_ms = ctx->acc_str_ms;
  ctx->last_cells = ctx->acc_cells;
  ctx->last_launches = ctx->acc_launches;
  ctx->last_launch_ms_sum = ctx->acc_launch_ms;
  ctx->last_launch_n = ctx->acc_launch_n;
  ctx->acc_stem_ms = ctx->acc_str_ms = ctx->acc_cells = ctx->acc_launch_ms = 0.0;
  ctx->acc_launch_n = ctx->acc_launches = 0;
  return SK_OK;
}

int sk_last_launch_ms(const sk_context* ctx, double* ms_sum, int32_t* n_launches) {
  if (!ctx) return SK_ERR_INVALID;
  if (ms_sum) *ms_sum = ctx->last_launch_ms_sum;
  if (n_launches) *n_launches = ctx->last_launch_n;
  return SK_OK;
}

int sk_last_classes(const sk_context* ctx, uint32_t* stem_maxk_mask, uint32_t* stem4d_mask) {
  if (!ctx) return SK_ERR_INVALID;
  if (stem_maxk_mask) *stem_maxk_mask = ctx->last_stem_classes;
  if (stem4d_mask) *stem4d_mask = ctx->last_s4d_classes;
  return SK_OK;
}

int32_t sk_last_gamma_shared(const sk_context* ctx) { return ctx ? ctx->last_gamma_shared : 0; }

int sk_last_la_protein(const sk_context* ctx, uint32_t* mask) {
  if (!ctx || !mask) return SK_ERR_INVALID;
  *mask = ctx->last_la_protein;
  return SK_OK;
}

int sk_last_string(const sk_context* ctx, int64_t pairs[3], int32_t waves[3]) {
  if (!ctx || !pairs || !waves) return SK_ERR_INVALID;
  for (int k = 0; k < 3; ++k) {
    pairs[k] = ctx->last_str_pairs[k];
    waves[k] = ctx->last_str_waves[k];
  }
  return SK_OK;
}

}  // extern "C"
