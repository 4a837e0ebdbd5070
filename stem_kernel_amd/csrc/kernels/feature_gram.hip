// Feature-vector Grams on CDNA4 (gfx950): the RBF, polynomial and sigmoid
// kernels of the reference's optimizer over libsvm feature vectors
// (optimizer/rbf_kernel.cpp, poly_kernel.cpp, sigmoid_kernel.cpp:
// calculate_matrix), K and its derivative matrices dK/dparam.
//
// Two kernels.  sk_feat_dot_kernel computes the dot matrix D = X Y^T once per
// (context, feature set or pair of sets); D does not depend on the kernel
// parameters and stays resident on the device, so every later call runs only
// sk_feat_apply_kernel, one pass over D that writes K and the 1 or 2 gradient
// matrices with the reference's formulas (host/feature_gram.h: feat_entry).
//
// The dot is exact, not fast: every output adds its terms x_k * y_k in
// ascending k from +0, the multiply and the add rounded separately
// (__dmul_rn, __dadd_rn; the file is also compiled with -ffp-contract=off), so
// D equals the reference's sparse merge bit for bit (the argument is in
// host/feature_gram.h).  That rules out MFMA, split-k and tree reductions on
// purpose: the Gram feeds the SMO solver and a conjugate gradient that
// amplifies rounding.
//
// sk_feat_dot_kernel: one workgroup of 256 threads per 64 x 64 tile of D, each
// thread a 4 x 4 block of accumulators in registers.  The X and Y panels of a
// k-slice of 16 columns (64 x 16 doubles each) are staged k-major through LDS,
// double-buffered (32 KiB): the next slice's global loads are issued before
// the current slice's products and stored after them, one barrier per slice.
// k only ever advances, so each accumulator sees its terms in order.  In the
// symmetric case only tiles with tile_i <= tile_j run, and the workgroup
// writes the mirror too (x_i . x_j and x_j . x_i are the same products in the
// same order, so a diagonal tile's two triangles are equal bits as computed).
// Edges: loads outside the arrays give +0 (adding x * 0 leaves a sum
// unchanged), stores are bounded; nothing is padded.
//
// sk_feat_apply_kernel: 32 x 32 tiles, four entries per thread, reads and
// writes coalesced; symmetric: tiles with tile_i <= tile_j, the mirror tile
// written through an LDS transpose, so K and G are exactly symmetric as the
// reference's are.  Memory-bound: n^2 doubles in, (1 + P) n^2 out.
// No atomics, no inline assembly.  Bounds: every load and store is checked
// against nx, ny, d in the kernel; the sizes are checked on the host first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../host/feature_gram.h"
#include "../host/runtime.h"
#include "stem_kernel.h"

namespace sk {

namespace {

constexpr int T = kFeatTile, S = kFeatSlice, R = kFeatReg;
static_assert(T == 64 && S == 16 && R == 4 && kFeatThreads == 256, "the thread maps below assume this shape");

template <bool SYM>
__global__ __launch_bounds__(kFeatThreads, 4) void sk_feat_dot_kernel(const double* __restrict__ X,
                                                                   const double* __restrict__ Y, int nx, int ny, int d,
                                                                   double* __restrict__ D) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (SYM && ti > tj) return;
  __shared__ double Xs[2][S][T];
  __shared__ double Ys[2][S][T];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;       // the thread's 4 x 4 block: rows ty*4.., columns tx*4..
  const int lr = tid >> 2, lk = (tid & 3) * 4;  // its share of a panel: row lr, columns lk..lk+3 of the slice
  const int64_t i0 = (int64_t)ti * T, j0 = (int64_t)tj * T;
  const int64_t xr = i0 + lr, yr = j0 + lr;
  const double* xrow = X + xr * d;
  const double* yrow = Y + yr * d;
  double acc[R][R];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < R; ++c) acc[r][c] = 0.0;

  double px[4], py[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + lk + q;
      px[q] = (xr < nx && k < d) ? xrow[k] : 0.0;
      py[q] = (yr < ny && k < d) ? yrow[k] : 0.0;
    }
  };
  auto stage = [&](int b) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      Xs[b][lk + q][lr] = px[q];
      Ys[b][lk + q][lr] = py[q];
    }
  };
  const int n_slices = (d + S - 1) / S;
  if (n_slices > 0) {
    fetch(0);
    stage(0);
  }
  __syncthreads();
  for (int s = 0; s < n_slices; ++s) {
    const int b = s & 1;
    if (s + 1 < n_slices) fetch((s + 1) * S);
#pragma unroll 2  // (a full unroll hoists every slice read: 256 VGPRs, one wave per SIMD)
    for (int kk = 0; kk < S; ++kk) {
      double a[R], y[R];
#pragma unroll
      for (int r = 0; r < R; ++r) a[r] = Xs[b][kk][ty * R + r];
#pragma unroll
      for (int c = 0; c < R; ++c) y[c] = Ys[b][kk][tx * R + c];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < R; ++c) acc[r][c] = __dadd_rn(acc[r][c], __dmul_rn(a[r], y[c]));
    }
    if (s + 1 < n_slices) stage(b ^ 1);  // (last read two slices ago, before the previous barrier)
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t i = i0 + ty * R + r;
#pragma unroll
    for (int c = 0; c < R; ++c) {
      const int64_t j = j0 + tx * R + c;
      if (i < nx && j < ny) {
        D[i * ny + j] = acc[r][c];
        if (SYM && ti != tj) D[j * ny + i] = acc[r][c];
      }
    }
  }
}

// dot(x, x) of every row, in order (the rectangular calls' RBF norms)
__global__ void sk_feat_norm_kernel(const double* __restrict__ X, int n, int d, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* x = X + (int64_t)i * d;
  double s = 0.0;
  for (int k = 0; k < d; ++k) s = __dadd_rn(s, __dmul_rn(x[k], x[k]));
  out[i] = s;
}

constexpr int AT = 32;  // feat_apply's tile edge

template <int KIND, bool SYM>
__global__ __launch_bounds__(256) void sk_feat_apply_kernel(const double* __restrict__ D, const double* __restrict__ dx,
                                                            const double* __restrict__ dy, int nx, int ny, int degree,
                                                            double p0, double p1, double* __restrict__ K,
                                                            double* __restrict__ G) {
  constexpr int NP = KIND == kFeatRbf ? 1 : 2;
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (SYM && ti > tj) return;
  __shared__ double tr[1 + NP][AT][AT + 1];
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int64_t i0 = (int64_t)ti * AT, j0 = (int64_t)tj * AT;
  const int64_t nn = (int64_t)nx * ny;
  const int64_t j = j0 + lx;
  const double djj = j < ny ? (SYM ? D[j * ny + j] : dy[j]) : 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ly + 8 * q;
    const int64_t i = i0 + r;
    double k = 0.0, g0 = 0.0, g1 = 0.0;
    if (i < nx && j < ny) {
      const double dii = SYM ? D[i * ny + i] : dx[i];
      feat_entry<KIND>(D[i * ny + j], dii, djj, degree, p0, p1, k, g0, g1);
      K[i * ny + j] = k;
      if (G) {
        G[i * ny + j] = g0;
        if (NP == 2) G[nn + i * ny + j] = g1;
      }
    }
    if (SYM && ti != tj) {
      tr[0][r][lx] = k;
      tr[1][r][lx] = g0;
      if (NP == 2) tr[2][r][lx] = g1;
    }
  }
  if (!SYM || ti == tj) return;  // (uniform per workgroup)
  __syncthreads();
  // the mirror tile: rows j0.., columns i0..
  const int64_t mc = i0 + lx;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ly + 8 * q;
    const int64_t mr = j0 + r;
    if (mr < ny && mc < nx) {
      K[mr * ny + mc] = tr[0][lx][r];
      if (G) {
        G[mr * ny + mc] = tr[1][lx][r];
        if (NP == 2) G[nn + mr * ny + mc] = tr[2][lx][r];
      }
    }
  }
}

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// A resident dot matrix: D (nx x ny) and, for a pair of sets, the row norms.
struct FeatDots {
  const sk_context* ctx;
  const sk_features *xs, *ys;  // ys null: symmetric
  int device;
  double *D, *dx, *dy;
};
std::mutex g_mu;
std::vector<FeatDots> g_dots;  // oldest first

void release(FeatDots& e) {
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) cur = -1;
  if (hipSetDevice(e.device) == hipSuccess) {
    for (double* p : {e.D, e.dx, e.dy})
      if (p) (void)hipFree(p);
  }
  if (cur >= 0) (void)hipSetDevice(cur);
}

template <int KIND>
void launch_apply(bool sym, dim3 grid, hipStream_t S_, const FeatDots& e, int nx, int ny, int degree, double p0,
                  double p1, double* K, double* G) {
  if (sym)
    hipLaunchKernelGGL((sk_feat_apply_kernel<KIND, true>), grid, dim3(256), 0, S_, e.D, e.dx, e.dy, nx, ny, degree, p0,
                       p1, K, G);
  else
    hipLaunchKernelGGL((sk_feat_apply_kernel<KIND, false>), grid, dim3(256), 0, S_, e.D, e.dx, e.dy, nx, ny, degree,
                       p0, p1, K, G);
}

}  // namespace

void feat_dots_forget(const sk_context* ctx, const sk_features* fs) {
  std::lock_guard<std::mutex> lock(g_mu);
  for (size_t k = 0; k < g_dots.size();) {
    FeatDots& e = g_dots[k];
    if ((ctx && e.ctx == ctx) || (fs && (e.xs == fs || e.ys == fs))) {
      release(e);
      g_dots.erase(g_dots.begin() + (long)k);
    } else {
      ++k;
    }
  }
}

}  // namespace sk

#define SK_FEAT_HIP(expr)                                                                             \
  do {                                                                                                \
    hipError_t _e = (expr);                                                                           \
    if (_e != hipSuccess)                                                                             \
      return sk::ctx_fail(ctx, SK_ERR_HIP, std::string(who) + ": " #expr ": " + hipGetErrorString(_e)); \
  } while (0)

namespace sk {
namespace {

// The resident D of (ctx, xs, ys), computed on the first call for it.  The
// calls are synchronous: the stream is drained before this returns a new D.
int feat_dots_get(const char* who, sk_context* ctx, const sk_features* xs, const sk_features* ys, FeatDots& out) {
  {
    std::lock_guard<std::mutex> lock(g_mu);
    for (const FeatDots& e : g_dots)
      if (e.ctx == ctx && e.xs == xs && e.ys == ys) {
        out = e;
        return SK_OK;
      }
  }
  hipStream_t S_ = ctx_stream(ctx);
  const int nx = xs->n, ny = ys ? ys->n : xs->n;
  const std::vector<int32_t> cols = feat_columns(xs, ys);
  const int d = (int)cols.size();
  DevBuf bx, by, bD, bnx, bny;
  const size_t xb = std::max<size_t>(16, (size_t)nx * d * 8), yb = std::max<size_t>(16, (size_t)ny * d * 8);
  std::vector<double> hx((size_t)nx * d), hy;
  feat_dense(xs, cols, hx.data());
  if (hipMalloc(&bx.p, xb) != hipSuccess || hipMalloc(&bD.p, std::max<size_t>(16, (size_t)nx * ny * 8)) != hipSuccess ||
      (ys && (hipMalloc(&by.p, yb) != hipSuccess || hipMalloc(&bnx.p, (size_t)nx * 8) != hipSuccess ||
              hipMalloc(&bny.p, (size_t)ny * 8) != hipSuccess))) {
    (void)hipGetLastError();
    return ctx_fail(ctx, SK_ERR_ALLOC, std::string(who) + ": device memory for the examples and the dot matrix");
  }
  if (!hx.empty()) SK_FEAT_HIP(hipMemcpyAsync(bx.p, hx.data(), hx.size() * 8, hipMemcpyHostToDevice, S_));
  if (ys) {
    hy.resize((size_t)ny * d);
    feat_dense(ys, cols, hy.data());
    if (!hy.empty()) SK_FEAT_HIP(hipMemcpyAsync(by.p, hy.data(), hy.size() * 8, hipMemcpyHostToDevice, S_));
  }
  const double* X = static_cast<const double*>(bx.p);
  const double* Y = ys ? static_cast<const double*>(by.p) : X;
  const dim3 grid((ny + T - 1) / T, (nx + T - 1) / T);
  SK_FEAT_HIP(lev_mark(ctx, S_));
  if (ys)
    hipLaunchKernelGGL((sk_feat_dot_kernel<false>), grid, dim3(kFeatThreads), 0, S_, X, Y, nx, ny, d,
                       static_cast<double*>(bD.p));
  else
    hipLaunchKernelGGL((sk_feat_dot_kernel<true>), grid, dim3(kFeatThreads), 0, S_, X, Y, nx, ny, d,
                       static_cast<double*>(bD.p));
  SK_FEAT_HIP(hipGetLastError());
  SK_FEAT_HIP(lev_mark(ctx, S_));
  if (ys) {
    SK_FEAT_HIP(lev_mark(ctx, S_));
    hipLaunchKernelGGL(sk_feat_norm_kernel, dim3((nx + 63) / 64), dim3(64), 0, S_, X, nx, d,
                       static_cast<double*>(bnx.p));
    hipLaunchKernelGGL(sk_feat_norm_kernel, dim3((ny + 63) / 64), dim3(64), 0, S_, Y, ny, d,
                       static_cast<double*>(bny.p));
    SK_FEAT_HIP(hipGetLastError());
    SK_FEAT_HIP(lev_mark(ctx, S_));
  }
  SK_FEAT_HIP(hipStreamSynchronize(S_));  // (the host images and the dense device copies die here)
  FeatDots e{ctx, xs, ys, ctx_device(ctx), static_cast<double*>(bD.p), static_cast<double*>(bnx.p),
             static_cast<double*>(bny.p)};
  bD.p = bnx.p = bny.p = nullptr;
  std::lock_guard<std::mutex> lock(g_mu);
  int mine = 0;
  for (const FeatDots& o : g_dots) mine += o.ctx == ctx;
  for (size_t k = 0; mine >= kFeatResident && k < g_dots.size(); ++k)
    if (g_dots[k].ctx == ctx) {  // the context's oldest
      release(g_dots[k]);
      g_dots.erase(g_dots.begin() + (long)k);
      break;
    }
  g_dots.push_back(e);
  out = e;
  return SK_OK;
}

int feat_gram_gpu(const char* who, sk_context* ctx, const sk_features* xs, const sk_features* ys, int kind, int degree,
                  const double* params, bool dots_only, double* out_k, double* out_g) {
  if (!ctx) return SK_ERR_INVALID;
  try {
    lev_reset(ctx);
    std::string err;
    if (!out_k) return ctx_fail(ctx, SK_ERR_INVALID, std::string(who) + ": null output");
    const int rc = feat_check(who, xs, ys, kind, degree, params, !dots_only, err);
    if (rc) return ctx_fail(ctx, rc, err);
    const int nx = xs->n, ny = ys ? ys->n : xs->n;
    if (nx == 0 || ny == 0) return SK_OK;
    SK_FEAT_HIP(hipSetDevice(ctx_device(ctx)));
    SK_FEAT_HIP(call_begin(ctx));
    hipStream_t S_ = ctx_stream(ctx);
    FeatDots e;
    const int rd = feat_dots_get(who, ctx, xs, ys, e);
    if (rd) return rd;
    const size_t nn8 = (size_t)nx * ny * 8;
    if (dots_only) {
      SK_FEAT_HIP(hipMemcpyAsync(out_k, e.D, nn8, hipMemcpyDeviceToHost, S_));
      SK_FEAT_HIP(hipStreamSynchronize(S_));
      SK_FEAT_HIP(lev_collect(ctx));
      return SK_OK;
    }
    const int np = out_g ? feat_n_params(kind) : 0;
    DevBuf out;
    if (hipMalloc(&out.p, nn8 * (size_t)(1 + np)) != hipSuccess) {
      (void)hipGetLastError();
      return ctx_fail(ctx, SK_ERR_ALLOC, std::string(who) + ": device memory for K and the gradient matrices");
    }
    double* K = static_cast<double*>(out.p);
    double* G = np ? K + (size_t)nx * ny : nullptr;
    const dim3 grid((ny + AT - 1) / AT, (nx + AT - 1) / AT);
    const double p0 = params[0], p1 = kind == kFeatRbf ? 0.0 : params[1];
    SK_FEAT_HIP(lev_mark(ctx, S_));
    switch (kind) {
      case kFeatRbf: launch_apply<kFeatRbf>(!ys, grid, S_, e, nx, ny, degree, p0, p1, K, G); break;
      case kFeatPoly: launch_apply<kFeatPoly>(!ys, grid, S_, e, nx, ny, degree, p0, p1, K, G); break;
      default: launch_apply<kFeatSigmoid>(!ys, grid, S_, e, nx, ny, degree, p0, p1, K, G);
    }
    SK_FEAT_HIP(hipGetLastError());
    SK_FEAT_HIP(lev_mark(ctx, S_));
    SK_FEAT_HIP(hipMemcpyAsync(out_k, K, nn8, hipMemcpyDeviceToHost, S_));
    if (np) SK_FEAT_HIP(hipMemcpyAsync(out_g, G, nn8 * (size_t)np, hipMemcpyDeviceToHost, S_));
    SK_FEAT_HIP(hipStreamSynchronize(S_));
    SK_FEAT_HIP(lev_collect(ctx));
    return SK_OK;
  } catch (const std::bad_alloc&) {
    return ctx_fail(ctx, SK_ERR_ALLOC, std::string(who) + ": host memory");
  }
}

}  // namespace
}  // namespace sk

extern "C" int sk_feature_dots(sk_context* ctx, const sk_features* xs, const sk_features* ys, double* out) {
  return sk::feat_gram_gpu("sk_feature_dots", ctx, xs, ys, 0, 0, nullptr, true, out, nullptr);
}

extern "C" int sk_feature_gram(sk_context* ctx, const sk_features* xs, int32_t kind, int32_t degree,
                               const double* params, double* out_k, double* out_g) {
  return sk::feat_gram_gpu("sk_feature_gram", ctx, xs, nullptr, kind, degree, params, false, out_k, out_g);
}

extern "C" int sk_feature_gram_cross(sk_context* ctx, const sk_features* test, const sk_features* train, int32_t kind,
                                     int32_t degree, const double* params, double* out_k) {
  if (!ctx) return SK_ERR_INVALID;
  if (!train) return sk::ctx_fail(ctx, SK_ERR_INVALID, "sk_feature_gram_cross: null training set");
  return sk::feat_gram_gpu("sk_feature_gram_cross", ctx, test, train, kind, degree, params, false, out_k, nullptr);
}
