// Planner of the protein local-alignment kinds (kernels/la_protein.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host/runtime_types.h"

namespace sk {

// Protein local-alignment kinds (la_protein.hip): pairs of two coded examples
// (every column one residue kind) go to the code kernel, the rest to the
// profile kernel; one launch each, results straight to out_dev.
int run_la_protein(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
                   const int32_t* x, const int32_t* y, int64_t n, double* out_dev) {
  const bool sw = kp->kind == SK_AA_LA_SW;
  static const bool host_stats = std::getenv("SK_HOST_STATS") != nullptr;
  const sk_dataset::ProtPack& PX = xs_->ppack;
  const sk_dataset::ProtPack& PY = ys_->ppack;
  // one pass: cells, the code pairs first (the permutation undone through
  // oidx), the longest y of each sort (the kernels' LDS)
  std::vector<uint8_t> codek((size_t)n);
  double cells = 0.0;
  int64_t n_code = 0;
  int32_t ymax_code = 0, ymax_prof = 0;
  for (int64_t k = 0; k < n; ++k) {
    const int32_t a = x[k], b = y[k];
    cells += (double)PX.ex_len[a] * (double)PY.ex_len[b];
    const uint8_t c = PX.ex_coded[a] & PY.ex_coded[b];
    codek[(size_t)k] = c;
    n_code += c;
    int32_t& m = c ? ymax_code : ymax_prof;
    m = std::max(m, PY.ex_len[b]);
  }
  ctx->last_cells = cells;
  // waves per workgroup: halved until the LDS fits, as run_bpla does
  const int len_code = (std::max(ymax_code, 64) + 1) & ~1, len_prof = (std::max(ymax_prof, 64) + 1) & ~1;
  int w_code = 4, w_prof = 4;
  while (w_code > 1 && sk::la_prot_code_lds_bytes(len_code, w_code) > 163840) w_code /= 2;
  while (w_prof > 1 && sk::la_prot_prof_lds_bytes(len_prof, w_prof) > 163840) w_prof /= 2;
  if (n_code && sk::la_prot_code_lds_bytes(len_code, w_code) > 163840)
    return fail(ctx, SK_ERR_UNSUPPORTED, "sequence too long for the protein LA kernel LDS (6,366 residues)");
  if (n_code < n && sk::la_prot_prof_lds_bytes(len_prof, w_prof) > 163840)
    return fail(ctx, SK_ERR_UNSUPPORTED, "alignment too long for the protein LA profile kernel LDS (1,326 columns)");
  std::vector<int32_t> px, py;
  std::vector<int64_t> oidx;
  const bool permute = n_code != 0 && n_code != n;
  if (permute) {
    px.resize((size_t)n);
    py.resize((size_t)n);
    oidx.resize((size_t)n);
    int64_t f = 0, g = n_code;
    for (int64_t k = 0; k < n; ++k) {
      const int64_t d = codek[(size_t)k] ? f++ : g++;
      px[(size_t)d] = x[k];
      py[(size_t)d] = y[k];
      oidx[(size_t)d] = k;
    }
    x = px.data();
    y = py.data();
  }
  const size_t nb = (size_t)n;
  int rc = ensure_work(ctx, 529 * 8 + 64 + nb * 8 + (permute ? nb * 8 : 0) + 8192);
  if (rc) return rc;
  // the call's inputs and zeroed counters go up in one copy (run_bpla)
  double* d_tb;
  unsigned long long* d_ctr;
  int32_t *d_px, *d_py;
  int64_t* d_oidx;
  auto lay = [&](Arena& U) {
    d_tb = U.take<double>(529);
    d_ctr = U.take<unsigned long long>(8);
    d_px = U.take<int32_t>(nb);
    d_py = U.take<int32_t>(nb);
    d_oidx = permute ? U.take<int64_t>(nb) : nullptr;
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
  hipStream_t S = ctx->stream;
  {
    thread_local std::vector<char> hb;
    hb.assign(up_bytes, 0);
    auto put = [&](const void* dptr, const void* src, size_t bytes) {
      if (bytes) std::memcpy(hb.data() + (static_cast<const char*>(dptr) - U.base), src, bytes);
    };
    put(d_tb, kp->aa_score_table, 529 * 8);
    put(d_px, x, nb * 4);
    put(d_py, y, nb * 4);
    if (permute) put(d_oidx, oidx.data(), nb * 8);
    if (ctx->async)
      SK_HIP(ctx, sk::up_copy(ctx, hb.data(), up_bytes, S));
    else
      SK_HIP(ctx, sk::h2d(ctx, U.base, hb.data(), up_bytes, S));
  }
  sk::LaProtLaunch T;
  T.xset = xs_->pdev;
  T.yset = ys_->pdev;
  T.table = d_tb;
  T.beta = kp->beta;
  T.gap = kp->gap;
  T.ext = kp->ext;
  T.beta_gap = std::exp(kp->beta * kp->gap);  // bpla_kernel.cpp:71-72
  T.beta_ext = std::exp(kp->beta * kp->ext);
  T.sw = sw ? 1 : 0;
  T.out = out_dev;
  SK_HIP(ctx, hipEventRecord(ctx->ev0, S));
  if (n_code) {
    sk::LaProtLaunch C = T;
    C.xs = d_px;
    C.ys = d_py;
    C.oidx = d_oidx;
    C.n_pairs = n_code;
    C.pair_counter = d_ctr;
    C.lds_max_len = len_code;
    const size_t lds = sk::la_prot_code_lds_bytes(len_code, w_code);
    const int per_cu = std::max(1, std::min<int>((int)(163840 / lds), 16 / w_code));
    const int64_t g = std::min<int64_t>((int64_t)ctx->n_cu * per_cu, (n_code + w_code - 1) / w_code);
    SK_HIP(ctx, sk::lev_mark(ctx, S));
    SK_HIP(ctx, sk::launch_la_prot_code(C, (int)g, w_code, S));
    SK_HIP(ctx, sk::lev_mark(ctx, S));
  }
  if (n_code < n) {
    sk::LaProtLaunch G = T;
    G.xs = d_px + n_code;
    G.ys = d_py + n_code;
    G.oidx = d_oidx ? d_oidx + n_code : nullptr;
    G.n_pairs = n - n_code;
    G.pair_counter = d_ctr + 1;
    G.lds_max_len = len_prof;
    const size_t lds = sk::la_prot_prof_lds_bytes(len_prof, w_prof);
    const int per_cu = std::max(1, std::min<int>((int)(163840 / lds), 8 / w_prof));
    const int64_t g = std::min<int64_t>((int64_t)ctx->n_cu * per_cu, (G.n_pairs + w_prof - 1) / w_prof);
    SK_HIP(ctx, sk::lev_mark(ctx, S));
    SK_HIP(ctx, sk::launch_la_prot_prof(G, (int)g, w_prof, S));
    SK_HIP(ctx, sk::lev_mark(ctx, S));
  }
  SK_HIP(ctx, hipEventRecord(ctx->ev1, S));
  ctx->last_launches = (n_code ? 1 : 0) + (n_code < n ? 1 : 0);
  ctx->last_la_protein = (n_code ? 1u : 0u) | (n_code < n ? 2u : 0u);
  SK_HIP(ctx, sk::call_finish(ctx, S, true, false));
  if (host_stats)
    fprintf(stderr, "[sk la protein] code kernel %lld pairs (%d waves), profile kernel %lld pairs (%d waves)\n",
            (long long)n_code, w_code, (long long)(n - n_code), w_prof);
  return SK_OK;
}

}  // namespace sk
