// Gradients of the protein local-alignment kernel: the C ABI calls
// (sk_la_protein_gradients*), the planner of kernels/la_protein_grad.hip and
// the host path.
//
// Reference: BPLAKernel<double,AAMData>::compute_gradients
// (bpla_kernel/bpla_kernel.cpp:385-401) over examples whose p_left and p_right
// are 0 and p_unpair 1 (what the noBP kernel scores), with alpha = 1.  The
// value is that function's return value, the reference's optimizer model, not
// operator()'s (sk_pairs with SK_AA_LA): its start states weight alignment
// starts differently, and it is not symmetric in (x, y).
//
// This file is built with -ffp-contract=off: the host path restates
// BPLA_Forward, BPLA_Backward and BPLA_ForwardBackword operation by operation
// and equals the reference bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "host/runtime.h"
#include "host/runtime_types.h"

namespace sk {
namespace {

constexpr int kNA = kAaSlots - 1;  // the 23 letters LAScore sums over
constexpr size_t kLaGradScratchBudget = (size_t)4 << 30;  // backward tables of the waves in flight

// ------------------------------------------------------------------ host path
enum { gM = 0, gIX, gIY, gLX, gLY, gRX, gRY, gN };

// LAScore::operator() (bpla_kernel.cpp:24-43) over two AAProfileSequence
// columns (24 float counts; the last slot, "other", is not summed)
inline double la_score(const double* tb, const float* xc, const float* yc) {
  double v = 0.0;
  float n = 0;
  for (int k = 0; k != kNA; ++k) {
    if (xc[k] == 0) continue;
    for (int l = 0; l != kNA; ++l) {
      if (yc[l] == 0) continue;
      n += xc[k] * yc[l];
      v += tb[k * kNA + l] * xc[k] * yc[l];
    }
  }
  return n == 0 ? 0.0 : v / n;
}

inline void update_alpha_beta(double& d_a, double& d_b, double a, double b, double w_pair, double w_unpair,
                              double v) {  // bpla_kernel.cpp:308-315
  d_a += b * w_pair * v;
  d_b += (a * w_pair + w_unpair) * v;
}

inline void update_beta_gap_ext(double& d_b, double& d_ge, double b, double ge, double v) {  // :317-324
  d_b += ge * v;
  d_ge += b * v;
}

// compute_gradients for one pair: full forward and backward tables, as the
// reference keeps them.  The weights are the constants p_left = p_right = 0,
// p_unpair = 1 (float, as in Data), alpha = 1.
double la_gradients_pair(const Example& X, const Example& Y, const double* tb, double beta, double gap, double ext,
                         double* d) {
  const int n = X.len, m = Y.len;
  const size_t W = (size_t)m + 1, C = ((size_t)n + 1) * W;
  const double alpha = 1.0;
  const float p_lr = 0.0f, p_un = 1.0f;
  const double beta_gap = std::exp(beta * gap);
  const double beta_ext = std::exp(beta * ext);
  std::vector<double> Fv(gN * C, 0.0), Bv(gN * C, 0.0), Wu(C, 0.0), Bs(C, 0.0);
  auto F = [&](int q, int i, int j) -> double& { return Fv[(size_t)q * C + (size_t)i * W + j]; };
  auto B = [&](int q, int i, int j) -> double& { return Bv[(size_t)q * C + (size_t)i * W + j]; };
  // the cell's score terms, once for the three passes (each pass of the
  // reference recomputes the same expressions)
  const double w_pair = p_lr * p_lr + p_lr * p_lr;
  for (int i = 1; i <= n; ++i)
    for (int j = 1; j <= m; ++j) {
      const double w_unpair = p_un * p_un * la_score(tb, X.aa_prof.data() + (size_t)(i - 1) * kAaSlots,
                                                     Y.aa_prof.data() + (size_t)(j - 1) * kAaSlots);
      Wu[(size_t)i * W + j] = w_unpair;
      Bs[(size_t)i * W + j] = std::exp(beta * (alpha * w_pair + w_unpair));
    }

  // ---- BPLA_Forward (:178-243)
  F(gM, 0, 0) = 1;
  F(gLX, 0, 0) = 1;
  F(gLY, 0, 0) = 1;
  for (int i = 1; i != n + 1; ++i) F(gLX, i, 0) += F(gLX, i - 1, 0);
  for (int j = 1; j != m + 1; ++j) F(gLY, 0, j) += F(gLY, 0, j - 1);
  for (int i = 1; i != n + 1; ++i) {
    for (int j = 1; j != m + 1; ++j) {
      const double beta_s = Bs[(size_t)i * W + j];
      F(gM, i, j) += beta_s * F(gM, i - 1, j - 1);
      F(gM, i, j) += beta_s * F(gIX, i - 1, j - 1);
      F(gM, i, j) += beta_s * F(gIY, i - 1, j - 1);
      F(gM, i, j) += beta_s * F(gLX, i - 1, j - 1);
      F(gM, i, j) += beta_s * F(gLY, i - 1, j - 1);

      F(gIX, i, j) += beta_gap * F(gM, i - 1, j);
      F(gIX, i, j) += beta_ext * F(gIX, i - 1, j);

      F(gIY, i, j) += beta_gap * F(gM, i, j - 1);
      F(gIY, i, j) += beta_gap * F(gIX, i, j - 1);
      F(gIY, i, j) += beta_ext * F(gIY, i, j - 1);

      F(gLX, i, j) += F(gLX, i - 1, 0);

      F(gLY, i, j) += F(gLX, i, j - 1);
      F(gLY, i, j) += F(gLY, i, j - 1);

      F(gRX, i, j) += F(gM, i - 1, j);
      F(gRX, i, j) += F(gRX, i - 1, j);

      F(gRY, i, j) += F(gM, i, j - 1);
      F(gRY, i, j) += F(gRX, i, j - 1);
      F(gRY, i, j) += F(gRY, i, j - 1);
    }
  }

  // ---- BPLA_Backward (:245-305); the closing loops over column 0 and row 0
  // (:297-303) only feed its return value, which compute_gradients drops
  B(gM, n, m) = 1;
  B(gRX, n, m) = 1;
  B(gRY, n, m) = 1;
  for (int i = n; i != 0; --i) {
    for (int j = m; j != 0; --j) {
      const double beta_s = Bs[(size_t)i * W + j];
      B(gM, i - 1, j - 1) += beta_s * B(gM, i, j);
      B(gIX, i - 1, j - 1) += beta_s * B(gM, i, j);
      B(gIY, i - 1, j - 1) += beta_s * B(gM, i, j);
      B(gLX, i - 1, j - 1) += beta_s * B(gM, i, j);
      B(gLY, i - 1, j - 1) += beta_s * B(gM, i, j);

      B(gM, i - 1, j) += beta_gap * B(gIX, i, j);
      B(gIX, i - 1, j) += beta_ext * B(gIX, i, j);

      B(gM, i, j - 1) += beta_gap * B(gIY, i, j);
      B(gIX, i, j - 1) += beta_gap * B(gIY, i, j);
      B(gIY, i, j - 1) += beta_ext * B(gIY, i, j);

      B(gLX, i - 1, 0) += B(gLX, i, j);

      B(gLX, i, j - 1) += B(gLY, i, j);
      B(gLY, i, j - 1) += B(gLY, i, j);

      B(gM, i - 1, j) += B(gRX, i, j);
      B(gRX, i - 1, j) += B(gRX, i, j);

      B(gM, i, j - 1) += B(gRY, i, j);
      B(gRX, i, j - 1) += B(gRY, i, j);
      B(gRY, i, j - 1) += B(gRY, i, j);
    }
  }

  // ---- BPLA_ForwardBackword (:325-383)
  d[0] = d[1] = d[2] = d[3] = 0.0;
  double& d_alpha = d[0];
  double& d_beta = d[1];
  double& d_gap = d[2];
  double& d_ext = d[3];
  for (int i = 1; i != n + 1; ++i) {
    for (int j = 1; j != m + 1; ++j) {
      const double w_unpair = Wu[(size_t)i * W + j];
      const double beta_s = Bs[(size_t)i * W + j];
      update_alpha_beta(d_alpha, d_beta, alpha, beta, w_pair, w_unpair, F(gM, i - 1, j - 1) * beta_s * B(gM, i, j));
      update_alpha_beta(d_alpha, d_beta, alpha, beta, w_pair, w_unpair, F(gIX, i - 1, j - 1) * beta_s * B(gM, i, j));
      update_alpha_beta(d_alpha, d_beta, alpha, beta, w_pair, w_unpair, F(gIY, i - 1, j - 1) * beta_s * B(gM, i, j));
      update_alpha_beta(d_alpha, d_beta, alpha, beta, w_pair, w_unpair, F(gLX, i - 1, j - 1) * beta_s * B(gM, i, j));
      update_alpha_beta(d_alpha, d_beta, alpha, beta, w_pair, w_unpair, F(gLY, i - 1, j - 1) * beta_s * B(gM, i, j));

      update_beta_gap_ext(d_beta, d_gap, beta, gap, F(gM, i - 1, j) * beta_gap * B(gIX, i, j));
      update_beta_gap_ext(d_beta, d_ext, beta, ext, F(gIX, i - 1, j) * beta_ext * B(gIX, i, j));

      update_beta_gap_ext(d_beta, d_gap, beta, gap, F(gM, i, j - 1) * beta_gap * B(gIY, i, j));
      update_beta_gap_ext(d_beta, d_gap, beta, gap, F(gIX, i, j - 1) * beta_gap * B(gIY, i, j));
      update_beta_gap_ext(d_beta, d_ext, beta, ext, F(gIY, i, j - 1) * beta_ext * B(gIY, i, j));
    }
  }
  return 1 + F(gM, n, m) + F(gRX, n, m) + F(gRY, n, m);
}

// the argument checks both calls share (before any work)
int check_args(sk_context* ctx, const sk_dataset* xs, const sk_dataset* ys, const sk_kernel_params* kp,
               const int32_t* x, const int32_t* y, int64_t n, const double* value, const double* grad) {
  if (!xs || !ys || !kp || n < 0 || (n > 0 && (!x || !y || !value || !grad)))
    return fail(ctx, SK_ERR_INVALID, "null argument or negative pair count");
  if (kp->kind != SK_AA_LA)
    return fail(ctx, SK_ERR_INVALID, "protein LA gradients need the kind SK_AA_LA (SK_AA_LA_SW has no gradient)");
  if ((!xs->ex.empty() && !ds_protein(xs)) || (!ys->ex.empty() && !ds_protein(ys)))
    return fail(ctx, SK_ERR_INVALID, "protein LA gradients on a dataset that is not protein");
  const int nx = (int)xs->ex.size(), ny = (int)ys->ex.size();
  for (int64_t k = 0; k < n; ++k)
    if (x[k] < 0 || x[k] >= nx || y[k] < 0 || y[k] >= ny) return fail(ctx, SK_ERR_RANGE, "pair index out of range");
  return SK_OK;
}

// --------------------------------------------------------------------- planner
// Pairs of two coded examples go to the code kernel, the rest to the profile
// kernel; one launch each, results by original index.  Scratch is (waves in
// flight) x (the largest pair's backward table): the grid shrinks until that
// fits kLaGradScratchBudget (a single wave's table may exceed it).
int la_gradients_gpu(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp, const int32_t* x,
                     const int32_t* y, int64_t n, double* value, double* grad) {
  const sk_dataset::ProtPack& PX = xs_->ppack;
  const sk_dataset::ProtPack& PY = ys_->ppack;
  std::vector<int32_t> px((size_t)n), py((size_t)n);
  std::vector<int64_t> oidx((size_t)n);
  int64_t n_code = 0;
  for (int64_t k = 0; k < n; ++k) n_code += PX.ex_coded[x[k]] & PY.ex_coded[y[k]];
  int32_t ymax[2] = {0, 0}, tmax[2] = {1, 1};  // [0] code, [1] profile
  double cells = 0.0;
  // the schedule counts a pair's steps in 32 bits (about |x| max(|y|, 64) / 64)
  for (int64_t k = 0; k < n; ++k)
    if (((double)PX.ex_len[x[k]] / 64.0 + 2.0) * (double)std::max(PY.ex_len[y[k]], 64) > 2.0e9)
      return fail(ctx, SK_ERR_UNSUPPORTED, "pair too large for the protein LA gradient kernels' step counter");
  {
    int64_t f = 0, g = n_code;
    for (int64_t k = 0; k < n; ++k) {
      const bool c = PX.ex_coded[x[k]] & PY.ex_coded[y[k]];
      const int64_t d = c ? f++ : g++;
      px[(size_t)d] = x[k];
      py[(size_t)d] = y[k];
      oidx[(size_t)d] = k;
      const int lx = PX.ex_len[x[k]], ly = PY.ex_len[y[k]];
      cells += (double)lx * (double)ly;
      ymax[c ? 0 : 1] = std::max(ymax[c ? 0 : 1], ly);
      tmax[c ? 0 : 1] = std::max(tmax[c ? 0 : 1], sk::bpla_steps(lx, ly));
    }
  }
  if (n_code && ymax[0] > sk::la_prot_grad_max_y(false))
    return fail(ctx, SK_ERR_UNSUPPORTED, "y sequence too long for the protein LA gradient code kernel's LDS");
  if (n_code < n && ymax[1] > sk::la_prot_grad_max_y(true))
    return fail(ctx, SK_ERR_UNSUPPORTED, "y alignment too long for the protein LA gradient profile kernel's LDS");
  SK_HIP(ctx, sk::call_begin(ctx));  // (synchronous: a fresh timing set)
  ctx->last_cells = cells;
  const size_t nb = (size_t)n;
  int rc = ensure_work(ctx, 529 * 8 + 64 + nb * (4 + 4 + 8 + 5 * 8) + 8192);
  if (rc) return rc;
  Arena A{static_cast<char*>(ctx->work), 0, ctx->work_bytes};
  double* d_tb = A.take<double>(529);
  unsigned long long* d_ctr = A.take<unsigned long long>(8);
  int32_t* d_px = A.take<int32_t>(nb);
  int32_t* d_py = A.take<int32_t>(nb);
  int64_t* d_oidx = A.take<int64_t>(nb);
  double* d_val = A.take<double>(nb);
  double* d_grad = A.take<double>(4 * nb);
  hipStream_t S = ctx->stream;
  SK_HIP(ctx, hipMemcpyAsync(d_tb, kp->aa_score_table, 529 * 8, hipMemcpyHostToDevice, S));
  SK_HIP(ctx, hipMemsetAsync(d_ctr, 0, 8 * sizeof(unsigned long long), S));
  SK_HIP(ctx, hipMemcpyAsync(d_px, px.data(), nb * 4, hipMemcpyHostToDevice, S));
  SK_HIP(ctx, hipMemcpyAsync(d_py, py.data(), nb * 4, hipMemcpyHostToDevice, S));
  SK_HIP(ctx, hipMemcpyAsync(d_oidx, oidx.data(), nb * 8, hipMemcpyHostToDevice, S));

  // the two launches' shapes: waves per workgroup halved until the LDS fits,
  // workgroups per CU by LDS, the grid by the pairs and the scratch budget
  struct Shape {
    int len = 64, waves = 4;
    int64_t grid = 0, bt = 0;
    size_t scratch = 0;
  } sh[2];
  for (int p = 0; p < 2; ++p) {
    const int64_t np = p == 0 ? n_code : n - n_code;
    if (!np) continue;
    Shape& H = sh[p];
    H.len = (std::max(ymax[p], 64) + 1) & ~1;
    auto lds = [&](int w) {
      return p == 0 ? sk::la_prot_grad_code_lds_bytes(H.len, w) : sk::la_prot_grad_prof_lds_bytes(H.len, w);
    };
    while (H.waves > 1 && lds(H.waves) > sk::kLaProtGradLds) H.waves /= 2;
    // resident workgroups per CU: by LDS, and 16 (code) or 8 (profile: 186 VGPRs) waves per CU
    const int per_cu = std::max(1, std::min<int>((int)(sk::kLaProtGradLds / lds(H.waves)), (p == 0 ? 16 : 8) / H.waves));
    H.bt = (int64_t)3 * 64 * tmax[p];
    H.grid = std::min<int64_t>((int64_t)ctx->n_cu * per_cu, (np + H.waves - 1) / H.waves);
    const int64_t by_budget = (int64_t)(kLaGradScratchBudget / ((size_t)H.bt * 8 * H.waves));
    if (by_budget < 1) {  // one wave at a time
      H.waves = 1;
      H.grid = std::max<int64_t>(1, std::min<int64_t>(H.grid, (int64_t)(kLaGradScratchBudget / ((size_t)H.bt * 8))));
    } else {
      H.grid = std::min(H.grid, by_budget);
    }
    H.scratch = (size_t)H.grid * H.waves * (size_t)H.bt * 8;
  }
  rc = ensure_scratch(ctx, std::max(sh[0].scratch, sh[1].scratch) + 64);  // (the launches run one after the other)
  if (rc) return rc;

  sk::LaProtGradLaunch T;
  T.xset = xs_->pdev;
  T.yset = ys_->pdev;
  T.table = d_tb;
  T.beta = kp->beta;
  T.gap = kp->gap;
  T.ext = kp->ext;
  T.beta_gap = std::exp(kp->beta * kp->gap);  // bpla_kernel.cpp:191-192
  T.beta_ext = std::exp(kp->beta * kp->ext);
  T.value = d_val;
  T.grad = d_grad;
  T.scratch = ctx->scratch;
  SK_HIP(ctx, hipEventRecord(ctx->ev0, S));
  if (n_code) {
    sk::LaProtGradLaunch C = T;
    C.xs = d_px;
    C.ys = d_py;
    C.oidx = d_oidx;
    C.n_pairs = n_code;
    C.pair_counter = d_ctr;
    C.lds_max_len = sh[0].len;
    C.bt_doubles = sh[0].bt;
    SK_HIP(ctx, sk::lev_mark(ctx, S));
    SK_HIP(ctx, sk::launch_la_prot_grad_code(C, (int)sh[0].grid, sh[0].waves, S));
    SK_HIP(ctx, sk::lev_mark(ctx, S));
  }
  if (n_code < n) {
    sk::LaProtGradLaunch G = T;
    G.xs = d_px + n_code;
    G.ys = d_py + n_code;
    G.oidx = d_oidx + n_code;
    G.n_pairs = n - n_code;
    G.pair_counter = d_ctr + 1;
    G.lds_max_len = sh[1].len;
    G.bt_doubles = sh[1].bt;
    SK_HIP(ctx, sk::lev_mark(ctx, S));
    SK_HIP(ctx, sk::launch_la_prot_grad_prof(G, (int)sh[1].grid, sh[1].waves, S));
    SK_HIP(ctx, sk::lev_mark(ctx, S));
  }
  SK_HIP(ctx, hipEventRecord(ctx->ev1, S));
  SK_HIP(ctx, hipMemcpyAsync(value, d_val, nb * 8, hipMemcpyDeviceToHost, S));
  SK_HIP(ctx, hipMemcpyAsync(grad, d_grad, 4 * nb * 8, hipMemcpyDeviceToHost, S));
  SK_HIP(ctx, hipStreamSynchronize(S));
  float ms = 0.f;
  SK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  ctx->last_stem_ms = ms;
  SK_HIP(ctx, sk::lev_collect(ctx));
  ctx->last_launches = (n_code ? 1 : 0) + (n_code < n ? 1 : 0);
  ctx->last_la_protein_grad = (n_code ? 1u : 0u) | (n_code < n ? 2u : 0u);
  return SK_OK;
}

}  // namespace
}  // namespace sk

extern "C" {

int sk_la_protein_gradients(sk_context* ctx, sk_dataset* xs, sk_dataset* ys, const sk_kernel_params* kp,
                            const int32_t* x, const int32_t* y, int64_t n_pairs, double* value, double* grad) {
  if (!ctx) return SK_ERR_INVALID;
  try {
    ctx->last_stem_ms = ctx->last_str_ms = ctx->last_cells = 0.0;
    ctx->last_launches = 0;
    sk::lev_reset(ctx);
    ctx->last_la_protein_grad = 0;
    int rc = sk::check_args(ctx, xs, ys, kp, x, y, n_pairs, value, grad);
    if (rc) return rc;
    rc = sk::check_set(ctx, xs);
    if (rc) return rc;
    rc = sk::check_set(ctx, ys);
    if (rc) return rc;
    if (n_pairs == 0) return SK_OK;
    return sk::la_gradients_gpu(ctx, xs, ys, kp, x, y, n_pairs, value, grad);
  } catch (const std::bad_alloc&) {
    return sk::fail(ctx, SK_ERR_ALLOC, "sk_la_protein_gradients: host memory");
  }
}

int sk_la_protein_gradients_host(sk_dataset* xs, sk_dataset* ys, const sk_kernel_params* kp, const int32_t* x,
                                 const int32_t* y, int64_t n_pairs, int32_t n_threads, double* value, double* grad) {
  if (n_threads < 0) return SK_ERR_INVALID;
  const int rc = sk::check_args(nullptr, xs, ys, kp, x, y, n_pairs, value, grad);
  if (rc || n_pairs == 0) return rc;
  int nt = n_threads ? n_threads : (int)std::max(1u, std::thread::hardware_concurrency());
  nt = (int)std::max<int64_t>(1, std::min<int64_t>(nt, n_pairs));
  std::atomic<int64_t> cursor{0};
  std::atomic<bool> oom{false};
  sk::run_pool(nt, [&] {
    for (int64_t k; (k = cursor.fetch_add(1)) < n_pairs && !oom.load(std::memory_order_relaxed);) {
      try {
        value[k] = sk::la_gradients_pair(xs->ex[x[k]], ys->ex[y[k]], kp->aa_score_table, kp->beta, kp->gap, kp->ext,
                                         grad + 4 * k);
      } catch (const std::bad_alloc&) {
        oom = true;
      }
    }
  });
  return oom ? SK_ERR_ALLOC : SK_OK;
}

int sk_la_protein_grad_shape(int32_t* max_y_code, int32_t* max_y_profile) {
  if (max_y_code) *max_y_code = sk::la_prot_grad_max_y(false);
  if (max_y_profile) *max_y_profile = sk::la_prot_grad_max_y(true);
  return SK_OK;
}

int sk_last_la_protein_grad(const sk_context* ctx, uint32_t* mask) {
  if (!ctx || !mask) return SK_ERR_INVALID;
  *mask = ctx->last_la_protein_grad;
  return SK_OK;
}

}  // extern "C"
