// Gradients of the DAG stem kernels with respect to loop_gap, beta, stack and
// covar: the C ABI calls (sk_stem_gradients*), their argument checks, the
// host path and the composite kinds' values.  The GPU planner is
// host/pairs_stem_grad.cpp, the kernel kernels/stem_grad.hip.
//
// Reference: StemKernel<ST,MData>::operator() (stem_kernel_lite/
// stem_kernel.cpp:14-95; node scores score_table.cpp:14-53, 118-201; edge
// scores :60-101), differentiated in forward mode: every DP quantity carries
// its value and one tangent per parameter, the product rule applied in the
// DP's own operation order.  The reference has no gradient of this kernel
// (stem_kernel/train.cpp calls an inside_outside that was never written).
//
// This file is built with -ffp-contract=off: the value's operations are the
// reference's own, in its order, so the host value equals it bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "host/runtime.h"
#include "host/runtime_types.h"
#include "ribosum85_60.inc"

namespace sk {
namespace {

constexpr int kRnaGap = 4;  // the gap column of a ProfileSequence row

// a DP quantity: the value and NP tangents
template <int NP>
struct Dual {
  double v;
  double t[NP];
};

// The per-call tables.  Tangent 0 is loop_gap; Su: 1 = beta; Si: 1 = stack,
// 2 = covar.
struct StemTables {
  bool subst = true;
  double co[256], dco[256];  // node-score table; Su: its d/dbeta
  std::vector<double> w, dw;  // loop_gap^k and k loop_gap^(k-1)
  double gap2 = 0.0, dgap2 = 0.0;
  unsigned band = 0;
};

StemTables make_tables(const sk_kernel_params* kp, int n_gpow) {
  StemTables T;
  T.subst = kind_subst(kp->kind);
  for (int k = 0; k < 256; ++k) {
    if (T.subst) {
      T.co[k] = std::exp(SK_RIBOSUM_P[k] * kp->beta);  // SubstNodeScore ctor (score_table.cpp:118-134)
      T.dco[k] = SK_RIBOSUM_P[k] * T.co[k];
    } else {
      T.co[k] = (k >> 4) == (k & 15) ? kp->stack : kp->covar;
      T.dco[k] = 0.0;
    }
  }
  T.w = gap_powers(kp->loop_gap, n_gpow);
  T.dw.assign(T.w.size(), 0.0);
  for (size_t k = 1; k < T.w.size(); ++k) T.dw[k] = (double)k * T.w[k - 1];
  T.gap2 = kp->loop_gap * kp->loop_gap;
  T.dgap2 = kp->loop_gap + kp->loop_gap;
  T.band = kp->len_band;
  return T;
}

// node_match_score (score_table.cpp:14-53 Simple, :162-201 Subst)
template <int NP>
Dual<NP> node_match(const StemTables& T, const Example& x, const Example& y, int i, int j) {
  Dual<NP> r;
  r.v = 0.0;
  for (int p = 0; p < NP; ++p) r.t[p] = 0.0;
  for (uint32_t a = x.bpf_off[i]; a != x.bpf_off[i + 1]; ++a) {
    const double cx = x.bpf_p[a];
    for (uint32_t b = y.bpf_off[j]; b != y.bpf_off[j + 1]; ++b) {
      const double cy = y.bpf_p[b];
      const int c = x.bpf_code[a] * 16 + y.bpf_code[b];
      r.v += T.co[c] * cx * cy;
      if (NP == 2)
        r.t[1] += T.dco[c] * cx * cy;
      else
        r.t[x.bpf_code[a] == y.bpf_code[b] ? 1 : 2] += cx * cy;
    }
  }
  const double nbp_x = x.prof5[(size_t)x.first[i] * 5 + kRnaGap];
  r.v += T.gap2 * y.weight[j] * nbp_x / (double)x.n_seqs;
  r.t[0] += T.dgap2 * y.weight[j] * nbp_x / (double)x.n_seqs;
  const double nbp_y = y.prof5[(size_t)y.first[j] * 5 + kRnaGap];
  r.v += T.gap2 * x.weight[i] * nbp_y / (double)y.n_seqs;
  r.t[0] += T.dgap2 * x.weight[i] * nbp_y / (double)y.n_seqs;
  return r;
}

// d += g * v_s * e_s, where v_s and e_s depend on loop_gap alone
template <int NP>
inline void add_gap_term(Dual<NP>& d, const Dual<NP>& g, double vs, double dvs, double es, double des) {
  d.v += g.v * vs * es;
  d.t[0] += (g.t[0] * vs + g.v * dvs) * es + g.v * vs * des;
  for (int p = 1; p < NP; ++p) d.t[p] += g.t[p] * vs * es;
}

// stem_kernel.cpp:14-95 over two examples; out[0] the value, out[1..NP] the
// tangents
template <int NP>
void stem_pair(const StemTables& T, const Example& x, const Example& y, double* out) {
  typedef Dual<NP> D;
  const int nx = x.n_nodes(), ny = y.n_nodes();
  for (int p = 0; p <= NP; ++p) out[p] = 0.0;
  if (nx == 0 || ny == 0) return;
  const size_t cells = (size_t)nx * ny;
  std::vector<D> K0(cells), G0(cells), K1(ny), G1(ny);
  D zero, one;
  zero.v = 0.0;
  one.v = 1.0;
  for (int p = 0; p < NP; ++p) zero.t[p] = one.t[p] = 0.0;
  std::fill(K1.begin(), K1.end(), zero);
  std::fill(G1.begin(), G1.end(), zero);
  const double* w = T.w.data();
  const double* dw = T.dw.data();
#define AT(M, a, b) M[(size_t)(a) * ny + (b)]
  for (int i = 0; i != nx; ++i) {
    const uint32_t xe0 = x.edge_off[i], xe1 = x.edge_off[i + 1];
    const int xlen = (int)(x.last[i] - x.first[i]);
    const double vsx = T.gap2 * x.weight[i], dvsx = T.dgap2 * x.weight[i];
    for (int j = 0; j != ny; ++j) {
      const uint32_t ye0 = y.edge_off[j], ye1 = y.edge_off[j + 1];
      if (xe0 == xe1 && ye0 == ye1) {
        AT(K0, i, j) = AT(G0, i, j) = one;
        continue;
      }
      K1[j] = G1[j] = zero;
      if (xe0 != xe1 && ye0 != ye1 &&
          (T.band == 0 || (unsigned)std::abs(xlen - (int)(y.last[j] - y.first[j])) <= T.band)) {
        const D vs = node_match<NP>(T, x, y, i, j);
        for (uint32_t ex = xe0; ex != xe1; ++ex) {
          for (uint32_t ey = ye0; ey != ye1; ++ey) {
            const uint32_t gx = x.edge_gaps[ex], gy = y.edge_gaps[ey];
            const double es = w[gx] * w[gy] * 1.0f * 1.0f;
            const double des = dw[gx] * w[gy] + w[gx] * dw[gy];
            const D& g = AT(G0, x.edge_to[ex], y.edge_to[ey]);
            const double gv = g.v * vs.v;
            const double v = gv * es;
            K1[j].v += v;
            G1[j].v += v;
            for (int p = 0; p < NP; ++p) {
              double d = (g.t[p] * vs.v + g.v * vs.t[p]) * es;
              if (p == 0) d += gv * des;
              K1[j].t[p] += d;
              G1[j].t[p] += d;
            }
          }
        }
      }
      const double vsy = T.gap2 * y.weight[j], dvsy = T.dgap2 * y.weight[j];
      for (uint32_t ey = ye0; ey != ye1; ++ey) {
        const uint32_t gy = y.edge_gaps[ey];
        const D& k1 = K1[y.edge_to[ey]];
        K1[j].v += k1.v;
        for (int p = 0; p < NP; ++p) K1[j].t[p] += k1.t[p];
        add_gap_term<NP>(G1[j], G1[y.edge_to[ey]], vsy, dvsy, w[gy] * 1.0f, dw[gy]);
      }
      AT(K0, i, j) = K1[j];
      AT(G0, i, j) = G1[j];
      for (uint32_t ex = xe0; ex != xe1; ++ex) {
        const uint32_t gx = x.edge_gaps[ex];
        const D& k0 = AT(K0, x.edge_to[ex], j);
        D& k = AT(K0, i, j);
        k.v += k0.v;
        for (int p = 0; p < NP; ++p) k.t[p] += k0.t[p];
        add_gap_term<NP>(AT(G0, i, j), AT(G0, x.edge_to[ex], j), vsx, dvsx, w[gx] * 1.0f, dw[gx]);
      }
    }
  }
  for (uint32_t a : x.roots)
    for (uint32_t b : y.roots) {
      const D& k = AT(K0, a, b);
      out[0] += k.v;
      for (int p = 0; p < NP; ++p) out[1 + p] += k.t[p];
    }
#undef AT
}

// StringKernel<double,MData>::operator() (stem_kernel_lite/string_kernel.cpp)
// over two examples: the string term of the composite kinds on the host path
double prof_subst(const double* st, const float* x, const float* y) {
  double v_c = 0.0;
  float n = 0;
  for (int i = 0; i != 4; ++i) {
    if (x[i] == 0) continue;
    for (int j = 0; j != 4; ++j) {
      if (y[j] == 0) continue;
      n += x[i] * y[j];
      v_c += st[i * 4 + j] * x[i] * y[j];
    }
  }
  return n == 0 ? 1.0 : v_c / n;
}

double string_pair(const sk_kernel_params* kp, const Example& xx, const Example& yy) {
  const bool ribosum = kind_subst(kp->kind);
  double st[16];
  for (int k = 0; k < 16; ++k)
    st[k] = ribosum ? std::exp(SK_RIBOSUM_S[k] * kp->alpha) : ((k >> 2) == (k & 3) ? kp->match : kp->mismatch);
  const double gap = kp->gap;
  const int sx = xx.len, sy = yy.len;
  const bool use_weight = xx.has_bp && yy.has_bp && sx > 0 && sy > 0;
  std::vector<double> K0p(sy + 1), G0p(sy + 1), K0c(sy + 1), G0c(sy + 1), K1(sy + 1, 0.0), G1(sy + 1, 0.0);
  K0p[0] = G0p[0] = 1.0;
  for (int j = 1; j != sy + 1; ++j) {
    K0p[j] = 1.0;
    G0p[j] = G0p[j - 1] * gap;
  }
  for (int i = 1; i != sx + 1; ++i) {
    K0c[0] = 1.0;
    G0c[0] = G0p[0] * gap;
    K1[0] = G1[0] = 0.0;
    for (int j = 1; j != sy + 1; ++j) {
      double v;
      if (use_weight)
        v = G0p[j - 1] * xx.pos_weight[i - 1] * yy.pos_weight[j - 1];
      else
        v = G0p[j - 1];
      v *= prof_subst(st, &xx.prof5[(size_t)(i - 1) * 5], &yy.prof5[(size_t)(j - 1) * 5]);
      K1[j] = v + K1[j - 1];
      G1[j] = v + G1[j - 1] * gap;
      K0c[j] = K1[j] + K0p[j];
      G0c[j] = G1[j] + G0p[j] * gap;
    }
    K0p.swap(K0c);
    G0p.swap(G0c);
  }
  return K0p[sy];
}

bool kind_ok(int k) {
  return k == SK_SU_STEM || k == SK_SI_STEM || k == SK_LSU_STEM || k == SK_SU_STEM_STR || k == SK_SI_STEM_STR ||
         k == SK_LSU_STEM_STR;
}

// the argument checks both calls share (before any work)
int check_args(sk_context* ctx, const sk_dataset* xs, const sk_dataset* ys, const sk_kernel_params* kp,
               const int32_t* x, const int32_t* y, int64_t n, const double* value, const double* grad) {
  if (!xs || !ys || !kp || n < 0 || (n > 0 && (!x || !y || !value || !grad)))
    return fail(ctx, SK_ERR_INVALID, "null argument or negative pair count");
  if (!kind_ok(kp->kind))
    return fail(ctx, SK_ERR_INVALID, "stem gradients need a DAG stem kind (SK_SU_STEM, SK_SI_STEM, SK_LSU_STEM or their + string kinds)");
  for (const sk_dataset* d : {xs, ys}) {
    if (ds_protein(d) || ds_pal(d)) return fail(ctx, SK_ERR_INVALID, "stem gradients on a dataset that is not RNA");
    for (const Example& X : d->ex)
      if (!X.has_bp) return fail(ctx, SK_ERR_INVALID, "stem gradients need examples built with use_bp");
  }
  const int nx = (int)xs->ex.size(), ny = (int)ys->ex.size();
  for (int64_t k = 0; k < n; ++k)
    if (x[k] < 0 || x[k] >= nx || y[k] < 0 || y[k] >= ny) return fail(ctx, SK_ERR_RANGE, "pair index out of range");
  return SK_OK;
}

// The kind's value and four-slot gradient row from the stem part's (Ks and
// its live tangents d[0..NP)) and the string term: the combine kernel's
// formulas (profile_string.hip) and their derivatives.
void finish_pair(const sk_kernel_params* kp, double ks, const double* d, double str, double* value, double* g) {
  const bool subst = kind_subst(kp->kind);
  g[0] = g[1] = g[2] = g[3] = 0.0;
  const int mode = combine_mode(kp->kind);
  if (mode == kCombineLogStem || mode == kCombineLogAdd) {
    const double lk = std::log(ks);
    const double v = kp->beta * lk + 0.0;
    *value = mode == kCombineLogStem ? v : v + (kp->alpha * std::log(str) + 0.0);
    if (ks == 0.0) {  // log 0: no derivative
      g[0] = g[1] = std::numeric_limits<double>::quiet_NaN();
    } else {
      g[0] = kp->beta * d[0] / ks;
      g[1] = lk + kp->beta * d[1] / ks;
    }
    return;
  }
  *value = mode == kCombineAdd ? ks + str : ks;
  g[0] = d[0];
  if (subst) {
    g[1] = d[1];
  } else {
    g[2] = d[1];
    g[3] = d[2];
  }
}

int max_gpow(const sk_dataset* xs, const sk_dataset* ys) {
  int m = 0;
  for (const sk_dataset* d : {xs, ys})
    for (const Example& X : d->ex) m = std::max(m, X.len);
  return 2 * m + 2;  // (every edge gap is below twice the longer example)
}

}  // namespace
}  // namespace sk

extern "C" {

int sk_stem_gradients(sk_context* ctx, sk_dataset* xs, sk_dataset* ys, const sk_kernel_params* kp,
                      const int32_t* x, const int32_t* y, int64_t n_pairs, double* value, double* grad) {
  if (!ctx) return SK_ERR_INVALID;
  try {
    ctx->last_stem_ms = ctx->last_str_ms = ctx->last_cells = 0.0;
    ctx->last_launches = 0;
    sk::lev_reset(ctx);
    ctx->last_stem_grad = 0;
    int rc = sk::check_args(ctx, xs, ys, kp, x, y, n_pairs, value, grad);
    if (rc) return rc;
    rc = sk::check_set(ctx, xs);
    if (rc) return rc;
    rc = sk::check_set(ctx, ys);
    if (rc) return rc;
    if (n_pairs == 0) return SK_OK;
    const size_t n = (size_t)n_pairs;
    // the string term of the + string kinds: the existing string path
    std::vector<double> str;
    if (sk::kind_has_str(kp->kind)) {
      str.resize(n);
      sk_kernel_params sp = *kp;
      sp.kind = sk::kind_subst(kp->kind) ? SK_SU_STR : SK_SI_STR;
      double* d = nullptr;
      SK_HIP(ctx, hipMalloc(&d, n * sizeof(double)));
      hipError_t e = sk::call_begin(ctx);
      rc = e != hipSuccess ? sk::fail(ctx, SK_ERR_HIP, hipGetErrorString(e))
                           : sk::run_dag_pairs(ctx, xs, ys, &sp, x, y, n_pairs, d);
      if (rc == SK_OK) {
        e = hipMemcpyAsync(str.data(), d, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = sk::fail(ctx, SK_ERR_HIP, hipGetErrorString(e));
      }
      (void)hipFree(d);
      if (rc) return rc;
      // (the call's timing below is the gradient launches' alone)
      ctx->last_stem_ms = ctx->last_str_ms = 0.0;
      ctx->last_launches = 0;
      sk::lev_reset(ctx);
    }
    std::vector<double> ks(n), d(4 * n);
    rc = sk::stem_gradients_gpu(ctx, xs, ys, kp, x, y, n_pairs, ks.data(), d.data());
    if (rc) return rc;
    const bool subst = sk::kind_subst(kp->kind);
    for (size_t k = 0; k < n; ++k) {
      // the kernel's row is in the four-slot layout: back to the live tangents
      const double live[3] = {d[4 * k], subst ? d[4 * k + 1] : d[4 * k + 2], d[4 * k + 3]};
      sk::finish_pair(kp, ks[k], live, str.empty() ? 0.0 : str[k], value + k, grad + 4 * k);
    }
    return SK_OK;
  } catch (const std::bad_alloc&) {
    return sk::fail(ctx, SK_ERR_ALLOC, "sk_stem_gradients: host memory");
  }
}

int sk_stem_gradients_host(sk_dataset* xs, sk_dataset* ys, const sk_kernel_params* kp, const int32_t* x,
                           const int32_t* y, int64_t n_pairs, int32_t n_threads, double* value, double* grad) {
  if (n_threads < 0) return SK_ERR_INVALID;
  const int rc = sk::check_args(nullptr, xs, ys, kp, x, y, n_pairs, value, grad);
  if (rc || n_pairs == 0) return rc;
  try {
    const sk::StemTables T = sk::make_tables(kp, sk::max_gpow(xs, ys));
    const bool str = sk::kind_has_str(kp->kind);
    int nt = n_threads ? n_threads : (int)std::max(1u, std::thread::hardware_concurrency());
    nt = (int)std::max<int64_t>(1, std::min<int64_t>(nt, n_pairs));
    std::atomic<int64_t> cursor{0};
    std::atomic<bool> oom{false};
    sk::run_pool(nt, [&] {
      for (int64_t k; (k = cursor.fetch_add(1)) < n_pairs && !oom.load(std::memory_order_relaxed);) {
        try {
          const sk::Example& X = xs->ex[x[k]];
          const sk::Example& Y = ys->ex[y[k]];
          double r[4];
          if (T.subst)
            sk::stem_pair<2>(T, X, Y, r);
          else
            sk::stem_pair<3>(T, X, Y, r);
          sk::finish_pair(kp, r[0], r + 1, str ? sk::string_pair(kp, X, Y) : 0.0, value + k, grad + 4 * k);
        } catch (const std::bad_alloc&) {
          oom = true;
        }
      }
    });
    return oom ? SK_ERR_ALLOC : SK_OK;
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
}

int sk_last_stem_grad(const sk_context* ctx, uint32_t* mask) {
  if (!ctx || !mask) return SK_ERR_INVALID;
  *mask = ctx->last_stem_grad;
  return SK_OK;
}

}  // extern "C"
