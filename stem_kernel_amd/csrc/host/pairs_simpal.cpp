// Planner of the palindrome kind (kernels/simpal.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "host/runtime_types.h"

namespace sk {

// Palindrome kind (simpal.hip): the pairs grouped by their y example, each
// group cut into work items of up to kSimpalWaves pairs, the items ordered by
// cost |P_y| * sum |P_x| (largest first); one launch, results straight to
// out_dev through oidx.
int run_simpal(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
               const int32_t* x, const int32_t* y, int64_t n, double* out_dev) {
  // the reference's int tolerance_ (simpal.cpp:231, 251): negative = every key pair counts
  if (!(kp->mismatch == std::floor(kp->mismatch)))
    return fail(ctx, SK_ERR_INVALID, "SK_SIMPAL: the tolerance (the mismatch field) must be an integer");
  if (n > (int64_t)INT32_MAX - 1) return fail(ctx, SK_ERR_UNSUPPORTED, "SK_SIMPAL: too many pairs in one call");
  if (ds_pal(xs_) && ds_pal(ys_) && xs_->ex[0].pal_seed != ys_->ex[0].pal_seed)
    return fail(ctx, SK_ERR_INVALID, "palindrome datasets of different seed_length");
  const int32_t tol = kp->mismatch < 0.0 ? 64 : (int32_t)std::min(kp->mismatch, 64.0);
  const std::vector<int32_t>& OX = xs_->spack.ex_off;
  const std::vector<int32_t>& OY = ys_->spack.ex_off;
  // libm's exp(-d) for d = 0..745, then 0 (exp(-746.0) underflows to 0)
  static const std::vector<double> exp_tab = [] {
    std::vector<double> t(sk::kSimpalExpN + 1, 0.0);
    for (int d = 0; d < sk::kSimpalExpN; ++d) t[d] = std::exp(-(double)d);
    return t;
  }();
  const size_t nb = (size_t)n;
  // the pairs grouped by y (a counting sort), inside a group by |P_x|,
  // largest first, then by their place in the call
  auto px_n = [&](int32_t k) { return OX[x[k] + 1] - OX[x[k]]; };
  const size_t n_y = ys_->ex.size();
  std::vector<int32_t> ord(nb);
  {
    std::vector<size_t> start(n_y + 1, 0);
    for (size_t k = 0; k < nb; ++k) ++start[(size_t)y[k] + 1];
    for (size_t g = 0; g < n_y; ++g) start[g + 1] += start[g];
    std::vector<size_t> fill(start.begin(), start.end() - 1);
    std::vector<uint64_t> key(nb);
    for (size_t k = 0; k < nb; ++k)
      key[fill[(size_t)y[k]]++] = (uint64_t)(0xffffffffu - (uint32_t)px_n((int32_t)k)) << 32 | (uint32_t)k;
    for (size_t g = 0; g < n_y; ++g)
      if (start[g + 1] - start[g] > 1) std::sort(key.begin() + start[g], key.begin() + start[g + 1]);
    for (size_t k = 0; k < nb; ++k) ord[k] = (int32_t)(key[k] & 0xffffffffu);
  }
  struct Item {
    int32_t first, count;
    double cost;
  };
  std::vector<Item> items;
  double terms = 0.0;
  for (size_t k = 0; k < nb;) {
    size_t e = k;
    double sx = 0.0;
    while (e < nb && e - k < (size_t)sk::kSimpalWaves && y[ord[e]] == y[ord[k]]) sx += (double)px_n(ord[e++]);
    const double c = sx * (double)(OY[y[ord[k]] + 1] - OY[y[ord[k]]]);
    items.push_back(Item{(int32_t)k, (int32_t)(e - k), c});
    terms += c;
    k = e;
  }
  ctx->last_cells = terms;
  std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.cost > b.cost; });
  const size_t ni = items.size();
  std::vector<int32_t> px(nb), py(nb), ifirst(ni + 1);
  std::vector<int64_t> oidx(nb);
  {
    size_t d = 0;
    for (size_t t = 0; t < ni; ++t) {
      ifirst[t] = (int32_t)d;
      for (int32_t q = 0; q < items[t].count; ++q, ++d) {
        const int32_t k = ord[(size_t)items[t].first + q];
        px[d] = x[k];
        py[d] = y[k];
        oidx[d] = k;
      }
    }
    ifirst[ni] = (int32_t)d;
  }
  const size_t ne = exp_tab.size();
  int rc = ensure_work(ctx, ne * 8 + 64 + nb * 16 + (ni + 1) * 4 + 8192);
  if (rc) return rc;
  // the call's inputs and the zeroed counter go up in one copy (run_bpla)
  double* d_tb;
  unsigned long long* d_ctr;
  int32_t *d_px, *d_py, *d_if;
  int64_t* d_oidx;
  auto lay = [&](Arena& U) {
    d_tb = U.take<double>(ne);
    d_ctr = U.take<unsigned long long>(8);
    d_px = U.take<int32_t>(nb);
    d_py = U.take<int32_t>(nb);
    d_if = U.take<int32_t>(ni + 1);
    d_oidx = U.take<int64_t>(nb);
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
    put(d_tb, exp_tab.data(), ne * 8);
    put(d_px, px.data(), nb * 4);
    put(d_py, py.data(), nb * 4);
    put(d_if, ifirst.data(), (ni + 1) * 4);
    put(d_oidx, oidx.data(), nb * 8);
    if (ctx->async)
      SK_HIP(ctx, sk::up_copy(ctx, hb.data(), up_bytes, S));
    else
      SK_HIP(ctx, sk::h2d(ctx, U.base, hb.data(), up_bytes, S));
  }
  sk::SimpalLaunch T;
  T.xset = xs_->sdev;
  T.yset = ys_->sdev;
  T.exp_tab = d_tb;
  T.tol = tol;
  T.item_first = d_if;
  T.n_items = (int32_t)ni;
  T.xs = d_px;
  T.ys = d_py;
  T.oidx = d_oidx;
  T.out = out_dev;
  T.item_counter = d_ctr;
  // four workgroups of kSimpalWaves waves per CU (4 waves per SIMD; their
  // LDS, 26.5 KB each, fits a CU's 160 KB)
  const int64_t g = std::min<int64_t>((int64_t)ctx->n_cu * 4, (int64_t)ni);
  SK_HIP(ctx, hipEventRecord(ctx->ev0, S));
  SK_HIP(ctx, sk::lev_mark(ctx, S));
  SK_HIP(ctx, sk::launch_simpal(T, (int)g, S));
  SK_HIP(ctx, sk::lev_mark(ctx, S));
  SK_HIP(ctx, hipEventRecord(ctx->ev1, S));
  ctx->last_launches = 1;
  SK_HIP(ctx, sk::call_finish(ctx, S, true, false));
  return SK_OK;
}

}  // namespace sk

extern "C" {

int sk_simpal_shape(int32_t* y_tile, int32_t* x_block) {
  if (y_tile) *y_tile = sk::kSimpalYTile;
  if (x_block) *x_block = sk::kSimpalXBlock;
  return SK_OK;
}

}  // extern "C"
