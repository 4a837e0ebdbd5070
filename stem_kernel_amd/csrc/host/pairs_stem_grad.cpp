// Planner of the stem gradient kernels (kernels/stem_grad.hip) behind
// sk_stem_gradients (host/stem_grad.cpp, which has checked the arguments).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "host/runtime.h"
#include "host/runtime_types.h"
#include "ribosum85_60.inc"

namespace sk {

// The stem part Ks of the pairs and d/d(loop_gap, beta, stack, covar), to the
// host buffers value[n] and grad[4 n].  One wavefront per pair, the pairs
// dealt cyclically to the waves, costliest first.  Per-wave scratch is
// (1 + NP) (slots + 3) rows of `stride` doubles; the grid is what the pairs,
// the CUs and half of the free device memory allow, and a call whose single
// wave does not fit that budget is refused before any launch.
int stem_gradients_gpu(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
                       const int32_t* x, const int32_t* y, int64_t n, double* value, double* grad) {
  const HostPack& PX = xs_->pack;
  const HostPack& PY = ys_->pack;
  const bool subst = kind_subst(kp->kind);
  const int T = subst ? 3 : 4;  // 1 + NP
  const size_t nb = (size_t)n;
  // costliest pairs first (ties by input order: deterministic)
  std::vector<int64_t> ord(nb);
  std::iota(ord.begin(), ord.end(), (int64_t)0);
  std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) {
    return (double)PX.ex_nl[x[a]] * PY.ex_nl[y[a]] > (double)PX.ex_nl[x[b]] * PY.ex_nl[y[b]];
  });
  std::vector<int32_t> px(nb), py(nb);
  int max_nly = 1;
  double cells = 0.0;
  for (size_t t = 0; t < nb; ++t) {
    px[t] = x[ord[t]];
    py[t] = y[ord[t]];
    max_nly = std::max(max_nly, PY.ex_nl[py[t]]);
    cells += (double)PX.ex_nl[px[t]] * (double)PY.ex_nl[py[t]];
  }
  const int64_t stride = ((int64_t)max_nly + 63) / 64 * 64;
  const int64_t wave_doubles = (int64_t)T * (PX.max_slots + 3) * stride;
  const size_t wg_bytes = (size_t)wave_doubles * 8 * sk::kStemGradWaves;
  size_t free_b = 0, total_b = 0;
  SK_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
  const size_t budget = std::min<size_t>((free_b + ctx->scratch_bytes) / 2, (size_t)32 << 30);
  if (wg_bytes > budget)  // (a workgroup's kStemGradWaves waves each hold the largest pair's rows)
    return fail(ctx, SK_ERR_UNSUPPORTED, "stem gradients: a pair's per-wave scratch does not fit the device memory budget");
  const int64_t by_mem = (int64_t)(budget / wg_bytes);
  const int64_t by_pairs = (n + sk::kStemGradWaves - 1) / sk::kStemGradWaves;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>({by_mem, by_pairs, (int64_t)ctx->n_cu * 8}));
  SK_HIP(ctx, sk::call_begin(ctx));  // (synchronous: a fresh timing set)
  ctx->last_cells = cells;
  int rc = ensure_scratch(ctx, (size_t)grid * wg_bytes + 64);
  if (rc) return rc;

  const int max_len = std::max(PX.max_len, PY.max_len);
  const int n_gp = max_len + 4;
  const size_t nnd = std::max<size_t>(PX.nd_a.size(), 1);
  rc = ensure_work(ctx, 2 * 256 * 8 + 2 * (size_t)n_gp * 8 + 6 * nnd * 8 + nb * (4 + 4 + 8 + 5 * 8) + 16 * 256);
  if (rc) return rc;
  Arena A{static_cast<char*>(ctx->work), 0, ctx->work_bytes};
  double* d_co = A.take<double>(256);
  double* d_dco = A.take<double>(256);
  double* d_gp = A.take<double>(n_gp);
  double* d_dgp = A.take<double>(n_gp);
  double* d_nd = A.take<double>(6 * nnd);
  int32_t* d_px = A.take<int32_t>(nb);
  int32_t* d_py = A.take<int32_t>(nb);
  int64_t* d_oidx = A.take<int64_t>(nb);
  double* d_val = A.take<double>(nb);
  double* d_grad = A.take<double>(4 * nb);

  // parameter tables and their tangents
  std::vector<double> co(256), dco(256, 0.0);
  for (int k = 0; k < 256; ++k) {
    if (subst) {
      co[k] = std::exp(SK_RIBOSUM_P[k] * kp->beta);
      dco[k] = SK_RIBOSUM_P[k] * co[k];
    } else {
      co[k] = (k >> 4) == (k & 15) ? kp->stack : kp->covar;
    }
  }
  const std::vector<double> gl = gap_powers(kp->loop_gap, n_gp);
  std::vector<double> dgl(gl.size(), 0.0);
  for (size_t k = 1; k < gl.size(); ++k) dgl[k] = (double)k * gl[k - 1];
  hipStream_t S = ctx->stream;
  SK_HIP(ctx, hipMemcpyAsync(d_co, co.data(), 256 * 8, hipMemcpyHostToDevice, S));
  SK_HIP(ctx, hipMemcpyAsync(d_dco, dco.data(), 256 * 8, hipMemcpyHostToDevice, S));
  SK_HIP(ctx, hipMemcpyAsync(d_gp, gl.data(), gl.size() * 8, hipMemcpyHostToDevice, S));
  SK_HIP(ctx, hipMemcpyAsync(d_dgp, dgl.data(), dgl.size() * 8, hipMemcpyHostToDevice, S));
  SK_HIP(ctx, hipMemcpyAsync(d_px, px.data(), nb * 4, hipMemcpyHostToDevice, S));
  SK_HIP(ctx, hipMemcpyAsync(d_py, py.data(), nb * 4, hipMemcpyHostToDevice, S));
  SK_HIP(ctx, hipMemcpyAsync(d_oidx, ord.data(), nb * 8, hipMemcpyHostToDevice, S));

  sk::StemGradPrep R;
  R.s = xs_->dev;
  R.gpow = d_gp;
  R.dgpow = d_dgp;
  R.gap2 = kp->loop_gap * kp->loop_gap;
  R.dgap2 = kp->loop_gap + kp->loop_gap;
  R.nd_L = d_nd;
  R.nd_dL = d_nd + nnd;
  R.nd_SL = d_nd + 2 * nnd;
  R.nd_dSL = d_nd + 3 * nnd;
  R.xr_SL = d_nd + 4 * nnd;
  R.xr_dSL = d_nd + 5 * nnd;

  sk::StemGradLaunch L;
  L.xset = xs_->dev;
  L.yset = ys_->dev;
  L.xr_SL = R.xr_SL;
  L.xr_dSL = R.xr_dSL;
  L.co = d_co;
  L.dco = d_dco;
  L.gpow = d_gp;
  L.dgpow = d_dgp;
  L.n_gpow = n_gp;
  L.gap2 = R.gap2;
  L.dgap2 = R.dgap2;
  L.band = kp->len_band;
  L.xs = d_px;
  L.ys = d_py;
  L.oidx = d_oidx;
  L.n_pairs = n;
  L.value = d_val;
  L.grad = d_grad;
  L.scratch = ctx->scratch;
  L.stride = stride;
  L.wave_doubles = wave_doubles;
  L.slots = PX.max_slots;
  SK_HIP(ctx, hipEventRecord(ctx->ev0, S));
  SK_HIP(ctx, sk::lev_mark(ctx, S));
  SK_HIP(ctx, sk::launch_stem_grad_prep(R, S));
  SK_HIP(ctx, sk::lev_mark(ctx, S));
  SK_HIP(ctx, sk::lev_mark(ctx, S));
  SK_HIP(ctx, sk::launch_stem_grad(L, subst, grid, S));
  SK_HIP(ctx, sk::lev_mark(ctx, S));
  SK_HIP(ctx, hipEventRecord(ctx->ev1, S));
  SK_HIP(ctx, hipMemcpyAsync(value, d_val, nb * 8, hipMemcpyDeviceToHost, S));
  SK_HIP(ctx, hipMemcpyAsync(grad, d_grad, 4 * nb * 8, hipMemcpyDeviceToHost, S));
  SK_HIP(ctx, hipStreamSynchronize(S));
  float ms = 0.f;
  SK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  ctx->last_stem_ms = ms;
  SK_HIP(ctx, sk::lev_collect(ctx));
  ctx->last_launches = 2;
  ctx->last_stem_grad = subst ? 1u : 2u;
  return SK_OK;
}

}  // namespace sk
