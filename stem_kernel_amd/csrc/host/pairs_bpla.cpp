// Planner of the BPLA kinds (kernels/bpla.hip) and the driver of their
// gradients (kernels/bpla_grad.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host/runtime_types.h"

namespace sk {

// BPLA kinds: one systolic launch (bpla.hip), result straight to out_dev.
int run_bpla(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
             const int32_t* x, const int32_t* y, int64_t n, double* out_dev) {
  const bool bp = kp->kind == SK_BPLA || kp->kind == SK_BPLA_SW;
  const bool sw = kp->kind == SK_BPLA_SW || kp->kind == SK_LA_SW;
  // SK_HOST_STATS: host time per phase (diagnostic)
  static const bool host_stats = std::getenv("SK_HOST_STATS") != nullptr;
  auto now_ms = [] {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  };
  const double tb0 = host_stats ? now_ms() : 0.0;
  double tb1 = tb0, tb2 = tb0;
  const HostPack& PX = xs_->pack;
  const HostPack& PY = ys_->pack;
  // per-example lengths and flags once (the pair loops below touch only
  // these small arrays, not the examples)
  const bool general_only = SK_KNOB("SK_BPLA_GENERAL") != nullptr;  // A/B switch
  auto ex_info = [&](const sk_dataset* d, const HostPack& H, std::vector<int32_t>& len,
                     std::vector<uint8_t>& ok, std::vector<uint8_t>& dy) {
    const size_t m = d->ex.size();
    len.resize(m);
    ok.resize(m);
    dy.resize(m);
    for (size_t i = 0; i < m; ++i) {
      len[i] = d->ex[i].len;
      ok[i] = !bp || d->ex[i].has_bp;  // BPLAScore reads p_left/p_right/p_unpair
      dy[i] = !general_only && H.ex_dyadic[i];
    }
  };
  std::vector<int32_t> lx, ly;
  std::vector<uint8_t> okx, oky, dyx, dyy;
  ex_info(xs_, PX, lx, okx, dyx);
  ex_info(ys_, PY, ly, oky, dyy);
  // one pass: cells, validity, fast flags, per-y counts of the fast pairs
  // (fast: both profiles dyadic -- the fast kernel with tabulated LAScore
  // factors; the rest the general one)
  std::vector<uint8_t> fastk((size_t)n);
  std::vector<int32_t> ycnt(ys_->ex.size(), 0);
  double cells = 0.0;
  int64_t n_fast = 0, distinct = 0;
  for (int64_t k = 0; k < n; ++k) {
    const int32_t a = x[k], b = y[k];
    if (!okx[a] || !oky[b])
      return fail(ctx, SK_ERR_INVALID, "BPLA with base pairs needs examples built with use_bp");
    cells += (double)lx[a] * (double)ly[b];
    const uint8_t f = dyx[a] & dyy[b];
    fastk[(size_t)k] = f;
    n_fast += f;
    if (f && ycnt[b]++ == 0) ++distinct;
  }
  ctx->last_cells = cells;
  // Fast pairs first, the permutation undone through oidx; fast pairs
  // grouped by y (a workgroup stages one y for all its waves) when the y's
  // repeat enough, else one pair per wave.  Items: runs of one y of at most
  // SK_BPLA_ITEM pairs (default 16 per wave of a full workgroup).
  std::vector<int32_t> px, py;
  std::vector<int64_t> oidx;
  constexpr int kItemWaves = 8;
  static const int item_max = SK_KNOB("SK_BPLA_ITEM") ? std::max(1, std::atoi(SK_KNOB("SK_BPLA_ITEM")))
                                                          : 16 * sk::kBplaItemsWavesMax;
  std::vector<int2> items;
  {
    const bool group = n_fast >= 4 * kItemWaves * std::max<int64_t>(distinct, 1) &&
                       !SK_KNOB("SK_BPLA_NO_ITEMS");
    const bool permute = n_fast != n || group;
    if (permute && n_fast) {
      px.resize((size_t)n);
      py.resize((size_t)n);
      oidx.resize((size_t)n);
      // fast pairs in y order (stable counting sort) or in call order, then
      // the general ones
      std::vector<int64_t> pos(ys_->ex.size() + 1, 0);
      if (group)
        for (size_t j = 0; j < ys_->ex.size(); ++j) pos[j + 1] = pos[j] + ycnt[j];
      int64_t f = 0, g = n_fast;
      for (int64_t k = 0; k < n; ++k) {
        const int64_t d = fastk[(size_t)k] ? (group ? pos[y[k]]++ : f++) : g++;
        px[(size_t)d] = x[k];
        py[(size_t)d] = y[k];
        oidx[(size_t)d] = k;
      }
      if (group)  // runs of one y
        for (int64_t a = 0; a < n_fast;) {
          int64_t b = a;
          while (b < n_fast && py[(size_t)b] == py[(size_t)a] && b - a < item_max) ++b;
          items.push_back(make_int2((int)a, (int)(b - a)));
          a = b;
        }
      x = px.data();
      y = py.data();
    }
  }
  if (host_stats) tb1 = now_ms();
  const bool permute = !oidx.empty();
  const size_t nb = (size_t)n;
  const size_t npx = PX.pos_prof.size(), npy = ys_ == xs_ ? 0 : PY.pos_prof.size();
  const size_t ntab = n_fast ? 2 * (npx + npy) : 0;
  int rc = ensure_work(ctx, 16 * 8 + nb * 8 + (permute ? nb * 8 : 0) + ntab * sizeof(sk::BplaPos) +
                                items.size() * sizeof(int2) + 8192);
  if (rc) return rc;
  // the call's host inputs and zeroed counters are laid out as on the device
  // and go up in ONE copy (separate small copies and a memset cost the
  // stream ~0.1 ms of gaps per call); asynchronous calls upload them on the
  // copy stream into a buffer of their own (up_reserve), overlapping the
  // previous call's kernels
  double* d_tb;
  unsigned long long* d_ctr;
  int32_t *d_px, *d_py;
  int64_t* d_oidx;
  int2* d_items;
  auto lay = [&](Arena& U) {
    d_tb = U.take<double>(16);
    d_ctr = U.take<unsigned long long>(8);
    d_px = U.take<int32_t>(nb);
    d_py = U.take<int32_t>(nb);
    d_oidx = permute ? U.take<int64_t>(nb) : nullptr;
    d_items = items.empty() ? nullptr : U.take<int2>(items.size());
  };
  Arena A{static_cast<char*>(ctx->work), 0, ctx->work_bytes};
  Arena U{nullptr, 0, 0};
  lay(U);  // (sizes only)
  const size_t up_bytes = U.off;
  if (ctx->async) {
    char* ub = nullptr;
    SK_HIP(ctx, sk::up_reserve(ctx, up_bytes, &ub));
    U = Arena{ub, 0, up_bytes};
    lay(U);
  } else {
    lay(A);
    U.base = A.base;
  }
  sk::BplaPos* d_tab = ntab ? A.take<sk::BplaPos>(ntab) : nullptr;
  hipStream_t S = ctx->stream;
  {
    thread_local std::vector<char> hb;
    hb.assign(up_bytes, 0);
    auto put = [&](const void* dptr, const void* src, size_t bytes) {
      if (bytes) std::memcpy(hb.data() + (static_cast<const char*>(dptr) - U.base), src, bytes);
    };
    put(d_tb, kp->score_table, 16 * 8);
    put(d_px, x, nb * 4);
    put(d_py, y, nb * 4);
    if (permute) put(d_oidx, oidx.data(), nb * 8);
    if (d_items) put(d_items, items.data(), items.size() * sizeof(int2));
    if (ctx->async)
      SK_HIP(ctx, sk::up_copy(ctx, hb.data(), up_bytes, S));
    else
      SK_HIP(ctx, sk::h2d(ctx, U.base, hb.data(), up_bytes, S));
  }
  sk::BplaLaunch T;
  T.xset = xs_->dev;
  T.yset = ys_->dev;
  T.table = d_tb;
  T.alpha = kp->alpha;
  T.beta = kp->beta;
  T.gap = kp->gap;
  T.ext = kp->ext;
  T.beta_gap = std::exp(kp->beta * kp->gap);  // bpla_kernel.cpp:70-71
  T.beta_ext = std::exp(kp->beta * kp->ext);
  T.sw = sw ? 1 : 0;
  T.bp = bp ? 1 : 0;
  T.oidx = d_oidx;
  T.out = out_dev;
  if (host_stats) tb2 = now_ms();
  SK_HIP(ctx, hipEventRecord(ctx->ev0, S));
  if (n_fast) {
    // x-role table of the x set, y-role table of the y set
    sk::BplaPos* tx = d_tab;           // [npx] x role | [npx] y role
    sk::BplaPos* ty = d_tab + npx;
    // the exp path's x operands carry beta (bpla_fast_chunk2)
    const double xscale = sw ? 1.0 : kp->beta;
    SK_HIP(ctx, sk::launch_bpla_tab(xs_->dev.pos_prof, xs_->dev.pos_lru, (int64_t)npx, d_tb, xscale, tx,
                                    d_tab + npx, S));
    if (npy) {
      ty = d_tab + 2 * npx + npy;      // [npy] x role (unused) | [npy] y role
      SK_HIP(ctx, sk::launch_bpla_tab(ys_->dev.pos_prof, ys_->dev.pos_lru, (int64_t)npy, d_tb, xscale,
                                      d_tab + 2 * npx, ty, S));
    }
    sk::BplaLaunch F = T;
    F.xtab = tx;
    F.ytab = ty;
    F.xs = d_px;
    F.ys = d_py;
    F.n_pairs = n_fast;
    F.pair_counter = d_ctr;
    F.lds_max_len = (std::max(PY.max_len, 64) + 1) & ~1;
    int w, per_cu;
    int64_t units;
    if (d_items) {  // y-grouped: workgroups of up to 16 waves sharing the y columns
      F.items = d_items;
      F.n_items = (int32_t)items.size();
      // pairs a wave streams back to back (SK_BPLA_CHUNK: 1..kBplaChunkMax)
      // (0: per item, as many as give each wave one chunk)
      F.chunk = 8;  // C4, items of 192 pairs: 7.99 ms per launch against 8.58 (4) and 8.97 (16)
      if (const char* e = SK_KNOB("SK_BPLA_CHUNK")) F.chunk = std::atoi(e);
      F.chunk = std::min(std::max(F.chunk, 0), sk::kBplaChunkMax);
      // waves per workgroup and workgroups per CU (SK_BPLA_IWAVES /
      // SK_BPLA_IWG: geometry experiments; the VGPR budget caps the waves
      // a SIMD holds, whatever is asked)
      // Default: one 16-wave workgroup per CU (C4: 11.1 against 11.7 ms
      // per launch for two 8-wave ones: the y columns staged once for 16
      // waves), halved while its LDS does not fit, the CU's 16 waves then
      // made up by more workgroups.
      static const int iw =
          SK_KNOB("SK_BPLA_IWAVES") ? std::atoi(SK_KNOB("SK_BPLA_IWAVES")) : sk::kBplaItemsWavesMax;
      static const int iwg = SK_KNOB("SK_BPLA_IWG") ? std::atoi(SK_KNOB("SK_BPLA_IWG")) : 0;
      w = std::min(std::max(iw, 1), sk::kBplaItemsWavesMax);
      while (w > 1 && sk::bpla_items_lds_bytes(F.lds_max_len, w) > 163840) w /= 2;
      const size_t l = sk::bpla_items_lds_bytes(F.lds_max_len, w);
      if (l > 163840) return fail(ctx, SK_ERR_UNSUPPORTED, "sequence too long for BPLA kernel LDS");
      per_cu = std::max(1, std::min<int>((int)(163840 / l), iwg > 0 ? iwg : std::max(1, sk::kBplaItemsWavesMax / w)));
      units = F.n_items;
    } else {
      const size_t wl = sk::bpla_fast_wave_lds_bytes(F.lds_max_len);
      if (wl > 163840) return fail(ctx, SK_ERR_UNSUPPORTED, "sequence too long for BPLA kernel LDS");
      // as many waves per CU as the per-wave LDS allows (<= 16), in
      // workgroups of up to 4
      static const int wcap =
          SK_KNOB("SK_BPLA_WAVES") ? std::atoi(SK_KNOB("SK_BPLA_WAVES")) : 16;
      const int per_cu_w =
          (int)std::max<size_t>(1, std::min<size_t>((size_t)wcap, (163840 - 2 * sk::kBplaExpLds) / wl));
      w = std::min(4, per_cu_w);
      per_cu = std::max(1, per_cu_w / w);
      units = (n_fast + w - 1) / w;
    }
    const int64_t g = std::min<int64_t>((int64_t)ctx->n_cu * per_cu, units);
    SK_HIP(ctx, sk::lev_mark(ctx, S));
    SK_HIP(ctx, sk::launch_bpla_fast(F, (int)g, w, S));
    SK_HIP(ctx, sk::lev_mark(ctx, S));
  }
  if (n_fast < n) {
    sk::BplaLaunch G = T;
    G.xs = d_px + n_fast;
    G.ys = d_py + n_fast;
    G.oidx = d_oidx ? d_oidx + n_fast : nullptr;
    G.n_pairs = n - n_fast;
    G.pair_counter = d_ctr + 1;
    G.lds_max_len = (std::max(PY.max_len, 64) + 1) & ~1;
    const int w = 4;
    const size_t lds = sk::bpla_lds_bytes(G, w);
    if (lds > 163840) return fail(ctx, SK_ERR_UNSUPPORTED, "sequence too long for BPLA kernel LDS");
    const int per_cu = std::max(1, std::min<int>((int)(163840 / lds), 8));
    const int64_t g = std::min<int64_t>((int64_t)ctx->n_cu * per_cu, (G.n_pairs + w - 1) / w);
    SK_HIP(ctx, sk::lev_mark(ctx, S));
    SK_HIP(ctx, sk::launch_bpla(G, (int)g, w, S));
    SK_HIP(ctx, sk::lev_mark(ctx, S));
  }
  SK_HIP(ctx, hipEventRecord(ctx->ev1, S));
  const double tb3 = host_stats ? now_ms() : 0.0;
  ctx->last_launches = (n_fast ? 1 : 0) + (n_fast < n ? 1 : 0);
  SK_HIP(ctx, sk::call_finish(ctx, S, true, false));
  if (host_stats)
    fprintf(stderr, "[sk bpla host] plan %.3f ms, uploads %.3f ms, launches %.3f ms, wait %.3f ms (GPU %.3f ms)\n",
            tb1 - tb0, tb2 - tb1, tb3 - tb2, now_ms() - tb3, ctx->async ? -1.0 : ctx->last_stem_ms);
  return SK_OK;
}

// BPLAKernel::compute_gradients over pairs (the bpla_optimizer's per-pair
// step, bpla_kernel.cpp:385-401, bpla_optimizer.cpp:52-255): batches bounded
// by scratch memory, one thread per pair.
int bpla_gradients(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
                   const int32_t* x, const int32_t* y, int64_t n, double* value, double* grad) {
  if (!ctx || !xs_ || !ys_ || !kp || (n > 0 && (!x || !y || !value || !grad)))
    return fail(ctx, SK_ERR_INVALID, "null argument");
  int rc = check_set(ctx, xs_);
  if (rc) return rc;
  rc = check_set(ctx, ys_);
  if (rc) return rc;
  if (ds_protein(xs_) || ds_protein(ys_))
    return fail(ctx, SK_ERR_INVALID, "BPLA gradients on a protein dataset");
  if (ds_pal(xs_) || ds_pal(ys_))
    return fail(ctx, SK_ERR_INVALID, "BPLA gradients on a palindrome dataset");
  if (n <= 0) return n < 0 ? fail(ctx, SK_ERR_INVALID, "negative pair count") : SK_OK;
  SK_HIP(ctx, sk::call_begin(ctx));  // (synchronous: a fresh timing set, not a pending one)
  for (int64_t k = 0; k < n; ++k) {
    if (x[k] < 0 || x[k] >= (int)xs_->ex.size() || y[k] < 0 || y[k] >= (int)ys_->ex.size())
      return fail(ctx, SK_ERR_INVALID, "pair index out of range");
    if (!xs_->ex[x[k]].has_bp || !ys_->ex[y[k]].has_bp)
      return fail(ctx, SK_ERR_INVALID, "BPLA gradients need examples built with use_bp");
  }
  size_t free_b = 0, total_b = 0;
  SK_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
  // one thread per pair, latency-bound: throughput grows with the pairs in
  // flight, so batches take most of the HBM
  const double budget = std::min(96e9, 0.6 * (double)free_b);
  rc = ensure_work(ctx, 16 * 8 + 4096);
  if (rc) return rc;
  double* d_tb = static_cast<double*>(ctx->work);
  hipStream_t S = ctx->stream;
  SK_HIP(ctx, hipMemcpyAsync(d_tb, kp->score_table, 16 * 8, hipMemcpyHostToDevice, S));
  // freed on every return path (an early SK_HIP return inside an optimizer
  // loop would otherwise leak both on each failing call)
  struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
      if (p) (void)hipFree(p);
    }
  } xy_buf, out_buf;
  SK_HIP(ctx, hipMalloc(&xy_buf.p, (size_t)2 * n * sizeof(int32_t)));
  SK_HIP(ctx, hipMalloc(&out_buf.p, (size_t)10 * n * sizeof(double)));
  int32_t* d_xy = static_cast<int32_t*>(xy_buf.p);
  double* d_out = static_cast<double*>(out_buf.p);
  SK_HIP(ctx, hipMemcpyAsync(d_xy, x, (size_t)n * 4, hipMemcpyHostToDevice, S));
  SK_HIP(ctx, hipMemcpyAsync(d_xy + n, y, (size_t)n * 4, hipMemcpyHostToDevice, S));
  double total_ms = 0.0;
  // pairs whose profiles are all dyadic take the wave-per-pair kernel (the
  // BPLA fast path's operand tables); the rest the thread-per-pair one
  const HostPack& PX = xs_->pack;
  const HostPack& PY = ys_->pack;
  std::vector<int32_t> wx, wy, gx, gy;
  std::vector<int64_t> wo, go;
  const bool general_only = SK_KNOB("SK_BPLA_GENERAL") != nullptr;  // A/B switch
  for (int64_t k = 0; k < n; ++k) {
    if (!general_only && PX.ex_dyadic[x[k]] && PY.ex_dyadic[y[k]]) {
      wx.push_back(x[k]);
      wy.push_back(y[k]);
      wo.push_back(k);
    } else {
      gx.push_back(x[k]);
      gy.push_back(y[k]);
      go.push_back(k);
    }
  }
  if (!wx.empty()) {
    const size_t nw = wx.size();
    const size_t npx = PX.pos_prof.size(), npy = ys_ == xs_ ? 0 : PY.pos_prof.size();
    const size_t ntab = 2 * (npx + npy);
    int tmax = 1, maxlen = 64;
    for (size_t k = 0; k < nw; ++k) {
      tmax = std::max(tmax, sk::bpla_steps(xs_->ex[wx[k]].len, ys_->ex[wy[k]].len));
      maxlen = std::max(maxlen, ys_->ex[wy[k]].len);
    }
    maxlen = (maxlen + 1) & ~1;
    const size_t wl = sk::bpla_grad_wave_lds_bytes(maxlen);
    if (wl + sk::kBplaExpLds > 163840)
      return fail(ctx, SK_ERR_UNSUPPORTED, "sequence too long for the BPLA gradient kernel LDS");
    const int per_cu_w = (int)std::max<size_t>(1, std::min<size_t>(16, (163840 - 2 * sk::kBplaExpLds) / wl));
    const int wpb = std::min(4, per_cu_w);
    const int64_t bt = (int64_t)3 * 64 * tmax;
    int64_t grid = (int64_t)ctx->n_cu * std::max(1, per_cu_w / wpb);
    grid = std::min<int64_t>(grid, std::max<int64_t>(1, ((int64_t)nw + wpb - 1) / wpb));
    grid = std::min<int64_t>(grid, std::max<int64_t>(1, (int64_t)(budget / (8.0 * bt * wpb))));
    DevBuf tab_buf, idx_buf;
    SK_HIP(ctx, hipMalloc(&tab_buf.p, ntab * sizeof(sk::BplaPos) + 64));
    SK_HIP(ctx, hipMalloc(&idx_buf.p, nw * (4 + 4 + 8) + 64));
    int32_t* d_wx = static_cast<int32_t*>(idx_buf.p);
    int32_t* d_wy = d_wx + nw;
    int64_t* d_wo = reinterpret_cast<int64_t*>(static_cast<char*>(idx_buf.p) + ((nw * 8 + 15) & ~size_t(15)));
    unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(d_tb + 16);  // after the table (work arena)
    SK_HIP(ctx, hipMemcpyAsync(d_wx, wx.data(), nw * 4, hipMemcpyHostToDevice, S));
    SK_HIP(ctx, hipMemcpyAsync(d_wy, wy.data(), nw * 4, hipMemcpyHostToDevice, S));
    SK_HIP(ctx, hipMemcpyAsync(d_wo, wo.data(), nw * 8, hipMemcpyHostToDevice, S));
    SK_HIP(ctx, hipMemsetAsync(d_cnt, 0, 8, S));
    sk::BplaPos* tabs = static_cast<sk::BplaPos*>(tab_buf.p);
    sk::BplaPos* tx = tabs;  // [npx] x role | [npx] y role (| [npy] x role | [npy] y role)
    sk::BplaPos* ty = tabs + npx;
    SK_HIP(ctx, sk::launch_bpla_tab(xs_->dev.pos_prof, xs_->dev.pos_lru, (int64_t)npx, d_tb, 1.0, tx,
                                    tabs + npx, S));
    if (npy) {
      ty = tabs + 2 * npx + npy;
      SK_HIP(ctx, sk::launch_bpla_tab(ys_->dev.pos_prof, ys_->dev.pos_lru, (int64_t)npy, d_tb, 1.0,
                                      tabs + 2 * npx, ty, S));
    }
    rc = ensure_scratch(ctx, (size_t)grid * wpb * (size_t)bt * 8 + 64);
    if (rc) return rc;
    sk::BplaGradLaunch W;
    W.xset = xs_->dev;
    W.yset = ys_->dev;
    W.table = d_tb;
    W.alpha = kp->alpha;
    W.beta = kp->beta;
    W.gap = kp->gap;
    W.ext = kp->ext;
    W.beta_gap = std::exp(kp->beta * kp->gap);  // bpla_kernel.cpp:188-189
    W.beta_ext = std::exp(kp->beta * kp->ext);
    W.xs = d_wx;
    W.ys = d_wy;
    W.n_pairs = (int64_t)nw;
    W.scratch = ctx->scratch;
    W.value = d_out;
    W.grad = d_out + n;
    W.xtab = tx;
    W.ytab = ty;
    W.pair_counter = d_cnt;
    W.oidx = d_wo;
    W.lds_max_len = maxlen;
    W.bt_doubles = bt;
    SK_HIP(ctx, hipEventRecord(ctx->ev0, S));
    SK_HIP(ctx, sk::launch_bpla_grad_wave(W, (int)grid, wpb, S));
    SK_HIP(ctx, hipEventRecord(ctx->ev1, S));
    SK_HIP(ctx, hipStreamSynchronize(S));
    float ms = 0.f;
    SK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    total_ms += ms;
  }
  // the thread-per-pair kernel over the remaining pairs, in place of (x, y)
  if (!wx.empty() && !gx.empty()) {
    SK_HIP(ctx, hipMemcpyAsync(d_xy, gx.data(), gx.size() * 4, hipMemcpyHostToDevice, S));
    SK_HIP(ctx, hipMemcpyAsync(d_xy + n, gy.data(), gy.size() * 4, hipMemcpyHostToDevice, S));
  }
  const int64_t ng = wx.empty() ? n : (int64_t)gx.size();
  const int32_t* hx = wx.empty() ? x : gx.data();
  const int32_t* hy = wx.empty() ? y : gy.data();
  // general results: in place when every pair is general, else in their own
  // region (values | grads of the general list), scattered on the host
  double* g_out = wx.empty() ? d_out : d_out + 5 * n;
  for (int64_t b0 = 0; b0 < ng && rc == SK_OK;) {
    int n1 = 1, m1 = 1;
    int64_t b1 = b0;
    while (b1 < ng) {
      const int a1 = std::max(n1, xs_->ex[hx[b1]].len + 1), c1 = std::max(m1, ys_->ex[hy[b1]].len + 1);
      if (b1 > b0 && (double)(b1 - b0 + 1) * sk::bpla_grad_pair_bytes(a1, c1) > budget) break;
      n1 = a1, m1 = c1, ++b1;
    }
    const int64_t cnt = b1 - b0;
    rc = ensure_scratch(ctx, (size_t)cnt * sk::bpla_grad_pair_bytes(n1, m1) + 64);
    if (rc) break;
    sk::BplaGradLaunch G;
    G.xset = xs_->dev;
    G.yset = ys_->dev;
    G.table = d_tb;
    G.alpha = kp->alpha;
    G.beta = kp->beta;
    G.gap = kp->gap;
    G.ext = kp->ext;
    G.beta_gap = std::exp(kp->beta * kp->gap);  // bpla_kernel.cpp:188-189
    G.beta_ext = std::exp(kp->beta * kp->ext);
    G.xs = d_xy + b0;
    G.ys = d_xy + n + b0;
    G.n_pairs = cnt;
    G.n1 = n1;
    G.m1 = m1;
    G.scratch = ctx->scratch;
    G.value = g_out + b0;
    G.grad = g_out + ng + 4 * b0;
    SK_HIP(ctx, hipEventRecord(ctx->ev0, S));
    SK_HIP(ctx, sk::launch_bpla_grad(G, S));
    SK_HIP(ctx, hipEventRecord(ctx->ev1, S));
    SK_HIP(ctx, hipStreamSynchronize(S));
    float ms = 0.f;
    SK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    total_ms += ms;
    b0 = b1;
  }
  if (rc == SK_OK) {
    hipError_t e = hipSuccess;
    if (!wx.empty()) {  // wave kernel: by original index
      std::vector<double> v(n), g(4 * (size_t)n);
      e = hipMemcpy(v.data(), d_out, (size_t)n * 8, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(g.data(), d_out + n, (size_t)4 * n * 8, hipMemcpyDeviceToHost);
      for (int64_t k : wo) {
        value[k] = v[k];
        for (int q = 0; q < 4; ++q) grad[4 * k + q] = g[4 * k + q];
      }
    }
    if (e == hipSuccess && ng) {
      std::vector<double> v(ng), g(4 * (size_t)ng);
      e = hipMemcpy(v.data(), g_out, (size_t)ng * 8, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(g.data(), g_out + ng, (size_t)4 * ng * 8, hipMemcpyDeviceToHost);
      for (int64_t t = 0; t < ng; ++t) {
        const int64_t k = wx.empty() ? t : go[t];
        value[k] = v[t];
        for (int q = 0; q < 4; ++q) grad[4 * k + q] = g[4 * t + q];
      }
    }
    if (e != hipSuccess) rc = fail(ctx, SK_ERR_HIP, hipGetErrorString(e));
  }
  ctx->last_stem_ms = total_ms;
  return rc;
}

}  // namespace sk
