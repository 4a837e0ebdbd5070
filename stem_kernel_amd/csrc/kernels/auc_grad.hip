// The optimizer's cross-validated AUC gradient on CDNA4 (gfx950): steps 4 and
// 5 of GradientComputation::compute (optimizer/gradient.cpp:107-156), one
// workgroup per (fold, C) problem over one Gram and its derivative matrices
// resident in device memory.
//
// Reference: find_support_vectors gradient.cpp:368-403, solve_d :405-456,
//   conjugate_gradient :622-644, calculate_gradient_c :511-547,
//   calculate_gradient_p :549-620.  The arithmetic contract is the one
//   csrc/host/auc_gradient.cpp restates, and every output is that file's bit
//   for bit: the conjugate gradient on the indefinite KKT system amplifies
//   rounding, so every sum here has the host's order, and every rounded
//   operation is an explicit __d*_rn, which the compiler does not contract.
//
// Schedule.  N = n_free + 1 is the side of the system.
//   1. Compaction: the free (0 < alpha < C) and bound (alpha >= C) examples of
//      the training list, T at a time: a ballot per wave, the waves' counts
//      through LDS, a running base -- a prefix scan that keeps training order.
//   2. P is materialised once, transposed (element (i, j) at [j N + i]), so
//      that in the product thread i's reads run beside its neighbours':
//      in LDS when N <= kAucLdsN (no bank conflicts: consecutive lanes on
//      consecutive doubles), else in the problem's device scratch (coalesced).
//   3. Product P v: one thread per row (rows beyond T loop per thread) adds
//      its row's terms in ascending j into a register, mul then add; v[j] is
//      an LDS broadcast.
//   4. The four dot products of a CG pass: each added by one lane in index
//      order from LDS, two at a time on lanes of different waves; a and B are
//      then computed by every thread from the same values (IEEE division).
//      The stopping test reads one LDS value, so it is uniform.
//   5. r, q, the rows of P' beta_u, dpsi: one thread per output element with
//      sequential terms.  The scalars' long chains (cg's n_test x n_bound
//      terms, the inner products) are staged through the two halves of an LDS
//      buffer: one lane adds kAucStage / 2 terms in order while the other
//      waves compute the next ones.
// No atomics, no inline assembly.  Bounds: every index is checked on the host
// before the launch, and the kernel leaves (n_free = -1) if its own count of
// free examples is not the host's, which sized LDS and the scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../host/auc_gradient.h"
#include "../host/runtime.h"

namespace sk {

namespace {

struct AucProb {
  double C, rho;
  int64_t scratch_off;  // doubles into the launch's scratch (second class)
  int64_t du_off;       // doubles into d_u
  int32_t train_off, n_train, test_off, n_test;
  int32_t list_off;     // into u_ty / u_k / c_ty (a multiple of 32)
  int32_t N;            // n_free + 1 as the host counted it
};
struct AucLaunch {
  const double* gram;
  const double* grads;
  int32_t n_params, n;
  const signed char* ypos;  // per example of the Gram: 1 when its label is > 0
  const int32_t* train;     // the problems' lists, concatenated
  const int32_t* test;
  const double* alpha;
  const double* delta;
  const AucProb* prob;
  const int32_t* which;  // the problems of this launch
  int32_t* u_ty;         // free examples: (Gram index << 1) | (y > 0)
  int32_t* u_k;          // ... and their positions in the training list
  int32_t* c_ty;         // bound examples
  double* scratch;
  double* cg;
  double* fg;
  double* du;
  sk_auc_info* info;
};

constexpr double kAucTol = 1e-10;

__device__ __forceinline__ int ysign(int ty) { return (ty & 1) ? 1 : -1; }

// One lane's sums in index order.  The adds are a dependent chain; the loads
// and products of eight terms are issued ahead of it.
__device__ __forceinline__ double seq_dot(const double* a, const double* b, int N) {
  double t = 0.0;
  int i = 0;
  for (; i + 8 <= N; i += 8) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = __dmul_rn(a[i + k], b[i + k]);
#pragma unroll
    for (int k = 0; k < 8; ++k) t = __dadd_rn(t, v[k]);
  }
  for (; i < N; ++i) t = __dadd_rn(t, __dmul_rn(a[i], b[i]));
  return t;
}

__device__ __forceinline__ double seq_add(double t, const double* a, int N) {
  int i = 0;
  for (; i + 8 <= N; i += 8) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = a[i + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) t = __dadd_rn(t, v[k]);
  }
  for (; i < N; ++i) t = __dadd_rn(t, a[i]);
  return t;
}

// acc + term(0) + term(1) + ... in that order: the terms are computed by all
// threads, kAucStage at a time, and added by thread 0 (whose return value is
// the sum; the other threads' is not)
// The stage is two halves: while thread 0 adds chunk c from one, the waves
// other than the first compute chunk c + 1 into the other; one barrier a chunk.
template <int T, class F>
__device__ __forceinline__ double seq_sum(double acc, int64_t count, F term, double* stage, int tid) {
  constexpr int H = kAucStage / 2;
  const int64_t chunks = (count + H - 1) / H;
  auto fill = [&](int64_t c) {
    const int64_t base = c * H;
    const int cnt = (int)(count - base < H ? count - base : H);
    double* buf = stage + (c & 1) * H;
    for (int e = tid - 64; e < cnt; e += T - 64) buf[e] = term(base + e);
  };
  if (chunks > 0 && tid >= 64) fill(0);
  __syncthreads();
  for (int64_t c = 0; c < chunks; ++c) {
    if (tid == 0) {
      const int64_t base = c * H;
      acc = seq_add(acc, stage + (c & 1) * H, (int)(count - base < H ? count - base : H));
    } else if (tid >= 64 && c + 1 < chunks) {
      fill(c + 1);
    }
    __syncthreads();
  }
  return acc;
}

// out = P v, P transposed at PT
template <int T>
__device__ __forceinline__ void product(const double* __restrict__ PT, const double* v, double* out, int N,
                                        int tid) {
  for (int i = tid; i < N; i += T) {
    double t = 0.0;
    const double* __restrict__ col = PT + i;
#pragma unroll 8
    for (int j = 0; j < N; ++j) t = __dadd_rn(t, __dmul_rn(col[(size_t)j * N], v[j]));
    out[i] = t;
  }
}

template <int T, bool LDSP>
__global__ void __launch_bounds__(T) sk_auc_grad_kernel(AucLaunch L) {
  constexpr int W = T / 64;
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ int32_t s_wf[W], s_wb[W];
  __shared__ double s_sc[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pi = L.which[blockIdx.x];
  const AucProb P = L.prob[pi];
  const int l = P.n_train, m = P.n_test, N = P.N, nsv = N - 1;
  const size_t n = (size_t)L.n;
  const double* __restrict__ K = L.gram;
  const int32_t* __restrict__ tr = L.train + P.train_off;
  const int32_t* __restrict__ ts = L.test + P.test_off;
  const double* __restrict__ alpha = L.alpha + P.train_off;
  const double* __restrict__ delta = L.delta + P.test_off;
  int32_t* u_ty = L.u_ty + P.list_off;
  int32_t* u_k = L.u_k + P.list_off;
  int32_t* c_ty = L.c_ty + P.list_off;
  const double C = P.C, b = P.rho;

  double* stage = sm;
  double* x = sm + kAucStage;
  double* r = x + N;
  double* w = r + N;
  double* z = w + N;
  double* PT = LDSP ? z + N : L.scratch + P.scratch_off;

  // ---- 1. compaction in training order
  int base_u = 0, base_c = 0;
  for (int k0 = 0; k0 < l; k0 += T) {
    const int k = k0 + tid;
    bool f = false, bd = false;
    int ty = 0;
    if (k < l) {
      const double a = alpha[k];
      const int t = tr[k];
      ty = (t << 1) | (L.ypos[t] ? 1 : 0);
      f = 0.0 < a && a < C;
      bd = !f && a >= C;
    }
    const unsigned long long mf = __ballot(f), mb = __ballot(bd);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane == 0) s_wf[wave] = __popcll(mf), s_wb[wave] = __popcll(mb);
    __syncthreads();
    int off_u = base_u, off_c = base_c, tot_u = 0, tot_c = 0;
#pragma unroll
    for (int q = 0; q < W; ++q) {
      if (q < wave) off_u += s_wf[q], off_c += s_wb[q];
      tot_u += s_wf[q], tot_c += s_wb[q];
    }
    // the lists have n_train slots, so a position is in range whatever alpha holds
    if (f) {
      const int pos = off_u + __popcll(mf & below);
      u_ty[pos] = ty, u_k[pos] = k;
    }
    if (bd) c_ty[off_c + __popcll(mb & below)] = ty;
    base_u += tot_u, base_c += tot_c;
    __syncthreads();
  }
  const int nc = base_c;
  if (base_u != nsv) {  // cannot happen: the host counted with the same tests
    if (tid == 0) {
      sk_auc_info I;
      I.n_free = -1, I.n_bound = nc, I.cg_iterations = 0, I.finite = 0;
      L.info[pi] = I;
    }
    return;
  }

  int products = 0;
  if (nsv > 0) {
    // ---- 2. P (transposed), r and x = 0
    for (int e = tid; e < N * N; e += T) {
      const int j = e / N, i = e - j * N;
      double v;
      if (i < nsv && j < nsv) {
        const int ti = u_ty[i], tj = u_ty[j];
        v = __dmul_rn((double)(ysign(ti) * ysign(tj)), K[(size_t)(ti >> 1) * n + (tj >> 1)]);
      } else if (i == nsv && j == nsv) {
        v = 0.0;
      } else {
        v = (double)(-ysign(u_ty[i < nsv ? i : j]));
      }
      PT[e] = v;
    }
    for (int i = tid; i < N; i += T) {
      double t = 0.0;
      if (i < nsv) {
        const int ti = u_ty[i];
        const double yi = (double)ysign(ti);
        const double* __restrict__ row = K + (size_t)(ti >> 1) * n;
        for (int j = 0; j < m; ++j) t = __dadd_rn(t, __dmul_rn(__dmul_rn(delta[j], yi), row[ts[j]]));
      } else {
        for (int j = 0; j < m; ++j) t = __dsub_rn(t, delta[j]);
      }
      r[i] = t;
      x[i] = 0.0;
    }
    __syncthreads();

    // ---- 3./4. conjugate_gradient from x = 0
    product<T>(PT, x, z, N, tid);
    __syncthreads();
    for (int i = tid; i < N; i += T) r[i] = __dsub_rn(r[i], z[i]);
    __syncthreads();
    if (tid == 0) s_sc[0] = seq_dot(r, r, N);
    __syncthreads();
    if (!(s_sc[0] < kAucTol)) {
      for (int i = tid; i < N; i += T) w[i] = -r[i];
      __syncthreads();
      product<T>(PT, w, z, N, tid);
      __syncthreads();
      products = 1;
      if (tid == 0) s_sc[1] = seq_dot(w, z, N);
      if (tid == 64) s_sc[2] = seq_dot(r, w, N);
      __syncthreads();
      double wz = s_sc[1];
      double a = __ddiv_rn(s_sc[2], wz);
      for (int i = tid; i < N; i += T) x[i] = __dadd_rn(x[i], __dmul_rn(a, w[i]));
      for (int pass = 0; pass < N; ++pass) {
        for (int i = tid; i < N; i += T) r[i] = __dsub_rn(r[i], __dmul_rn(a, z[i]));
        __syncthreads();
        if (tid == 0) s_sc[0] = seq_dot(r, r, N);
        if (tid == 64) s_sc[3] = seq_dot(r, z, N);
        __syncthreads();
        if (s_sc[0] < kAucTol) break;
        const double B = __ddiv_rn(s_sc[3], wz);
        for (int i = tid; i < N; i += T) w[i] = __dadd_rn(-r[i], __dmul_rn(B, w[i]));
        __syncthreads();
        product<T>(PT, w, z, N, tid);
        __syncthreads();
        ++products;
        if (tid == 0) s_sc[1] = seq_dot(w, z, N);
        if (tid == 64) s_sc[2] = seq_dot(r, w, N);
        __syncthreads();
        wz = s_sc[1];
        a = __ddiv_rn(s_sc[2], wz);
        for (int i = tid; i < N; i += T) x[i] = __dadd_rn(x[i], __dmul_rn(a, w[i]));
      }
    }
    __syncthreads();
    // d_u out; z = alpha_u for step 5
    for (int i = tid; i < N; i += T) {
      L.du[P.du_off + i] = x[i];
      z[i] = i < nsv ? alpha[u_k[i]] : 0.0;
    }
    // ---- 5a. q of calculate_gradient_c in r
    for (int i = tid; i < N; i += T) {
      double t = 0.0;
      if (i < nsv) {
        const int ti = u_ty[i];
        const double* __restrict__ row = K + (size_t)(ti >> 1) * n;
        for (int j = 0; j < nc; ++j) {
          const int tj = c_ty[j];
          t = __dsub_rn(t, __dmul_rn((double)(ysign(ti) * ysign(tj)), row[tj >> 1]));
        }
      } else {
        for (int j = 0; j < nc; ++j) t = __dadd_rn(t, (double)ysign(c_ty[j]));
      }
      r[i] = t;
    }
    __syncthreads();
  }

  // ---- 5b. cg
  double acc = 0.0;
  if (nsv > 0 && tid == 0) acc = __dadd_rn(acc, seq_dot(x, r, N));
  acc = seq_sum<T>(acc, (int64_t)m * nc,
                   [&](int64_t e) {
                     const int i = (int)(e / nc), j = (int)(e - (int64_t)i * nc);
                     const int tj = c_ty[j];
                     return __dmul_rn(__dmul_rn(delta[i], (double)ysign(tj)), K[(size_t)ts[i] * n + (tj >> 1)]);
                   },
                   stage, tid);
  if (tid == 0) L.cg[pi] = acc;

  // ---- 5c. fg[p]
  for (int p = 0; p < L.n_params; ++p) {
    const double* __restrict__ g = L.grads + (size_t)p * n * n;
    double ret = 0.0;
    if (nsv > 0) {
      for (int i = tid; i < N; i += T) {
        double t = 0.0, s = 0.0;
        if (i < nsv) {
          const int ti = u_ty[i];
          const double* __restrict__ row = g + (size_t)(ti >> 1) * n;
          for (int j = 0; j < nc; ++j) {
            const int tj = c_ty[j];
            t = __dsub_rn(t, __dmul_rn(__dmul_rn((double)(ysign(ti) * ysign(tj)), row[tj >> 1]), C));
          }
          for (int j = 0; j < nsv; ++j) {
            const int tj = u_ty[j];
            s = __dadd_rn(s, __dmul_rn(__dmul_rn((double)(ysign(ti) * ysign(tj)), row[tj >> 1]), z[j]));
          }
        } else {
          for (int j = 0; j < nsv; ++j) s = __dadd_rn(s, __dmul_rn(0.0, z[j]));
        }
        s = __dadd_rn(s, __dmul_rn(0.0, b));
        w[i] = __dmul_rn(x[i], __dsub_rn(t, s));
      }
      __syncthreads();
      if (tid == 0) ret = __dadd_rn(ret, seq_add(0.0, w, N));
    }
    const double t2 = seq_sum<T>(0.0, (int64_t)l + 1,
                                 [&](int64_t e) {
                                   if (e == l) return __dmul_rn(0.0, b);
                                   const int t = tr[e];
                                   const double yj = L.ypos[t] ? 1.0 : -1.0;
                                   double dpsi = 0.0;
                                   for (int i = 0; i < m; ++i)
                                     dpsi = __dadd_rn(dpsi, __dmul_rn(__dmul_rn(delta[i], yj), g[(size_t)ts[i] * n + t]));
                                   return __dmul_rn(dpsi, alpha[e]);
                                 },
                                 stage, tid);
    if (tid == 0) L.fg[(size_t)pi * L.n_params + p] = __dadd_rn(ret, t2);
  }
  if (tid == 0) {
    sk_auc_info I;
    I.n_free = nsv, I.n_bound = nc, I.cg_iterations = products, I.finite = 0;  // finite: the host fills it in
    L.info[pi] = I;
  }
}

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

size_t lds_bytes(int N, bool ldsp) {
  return 8 * ((size_t)kAucStage + 4 * (size_t)N + (ldsp ? (size_t)N * N : 0));
}

}  // namespace
}  // namespace sk

#define SK_AUC_HIP(expr)                                                                                    \
  do {                                                                                                      \
    hipError_t _e = (expr);                                                                                 \
    if (_e != hipSuccess)                                                                                   \
      return sk::ctx_fail(ctx, SK_ERR_HIP, std::string("sk_auc_gradient_batch: " #expr ": ") + hipGetErrorString(_e)); \
  } while (0)

extern "C" int sk_auc_gradient_batch(sk_context* ctx, const double* gram, const double* grads, int32_t n_params,
                                     int32_t n, const double* labels, const sk_auc_problem* problems,
                                     int32_t n_problems, double* cg_out, double* fg_out, double* d_u_out,
                                     sk_auc_info* info) {
  if (!ctx) return SK_ERR_INVALID;
  try {
    sk::lev_reset(ctx);
    std::string err;
    std::vector<int32_t> nf, nb;
    const int rc = sk::auc_check_batch(gram, grads, n_params, n, labels, problems, n_problems, cg_out, fg_out,
                                       info, sk::kAucMaxN, nf, nb, err);
    if (rc) return sk::ctx_fail(ctx, rc, err);
    if (n_problems == 0) return SK_OK;

    // host images: labels' signs, the lists concatenated, the descriptors, the two classes
    std::vector<signed char> ypos(n);
    for (int32_t k = 0; k < n; ++k) ypos[k] = labels[k] > 0 ? 1 : 0;
    int64_t sum_train = 0, sum_test = 0, sum_list = 0, sum_du = 0;
    for (int p = 0; p < n_problems; ++p) {
      sum_train += problems[p].n_train;
      sum_test += problems[p].n_test;
      sum_list += (problems[p].n_train + 31) & ~31;
      sum_du += problems[p].n_train + 1;
    }
    if (sum_list > INT32_MAX || sum_test > INT32_MAX)
      return sk::ctx_fail(ctx, SK_ERR_UNSUPPORTED, "sk_auc_gradient_batch: over 2^31 list entries in one call");
    std::vector<int32_t> train((size_t)sum_train), test((size_t)sum_test);
    std::vector<double> alpha((size_t)sum_train), delta((size_t)sum_test);
    std::vector<sk::AucProb> prob(n_problems);
    std::vector<int32_t> small, big;
    std::vector<int64_t> du_off(n_problems);
    {
      int32_t to = 0, so = 0, lo = 0;
      int64_t dv = 0;
      for (int p = 0; p < n_problems; ++p) {
        const sk_auc_problem& P = problems[p];
        sk::AucProb& D = prob[p];
        D.C = P.C, D.rho = P.rho, D.scratch_off = 0, D.du_off = du_off[p] = dv;
        D.train_off = to, D.n_train = P.n_train, D.test_off = so, D.n_test = P.n_test;
        D.list_off = lo, D.N = nf[p] + 1;
        std::memcpy(train.data() + to, P.train, (size_t)P.n_train * 4);
        std::memcpy(alpha.data() + to, P.alpha, (size_t)P.n_train * 8);
        std::memcpy(test.data() + so, P.test, (size_t)P.n_test * 4);
        std::memcpy(delta.data() + so, P.delta, (size_t)P.n_test * 8);
        to += P.n_train, so += P.n_test, lo += (P.n_train + 31) & ~31, dv += P.n_train + 1;
        (D.N <= sk::kAucLdsN ? small : big).push_back(p);
      }
    }
    // the second class in launches whose P scratches share the budget, largest systems first
    std::sort(big.begin(), big.end(), [&](int a, int c) { return prob[a].N != prob[c].N ? prob[a].N > prob[c].N : a < c; });
    std::vector<std::pair<int, int>> waves;  // [first, last) into big
    int64_t scratch_max = 0;
    for (size_t at = 0; at < big.size();) {
      int64_t used = 0;
      size_t end = at;
      while (end < big.size()) {
        const int64_t need = (int64_t)prob[big[end]].N * prob[big[end]].N;
        if (end > at && (used + need) * 8 > sk::kAucScratchBudget) break;
        prob[big[end]].scratch_off = used;
        used += need;
        ++end;
      }
      scratch_max = std::max(scratch_max, used);
      waves.emplace_back((int)at, (int)end);
      at = end;
    }
    std::vector<int32_t> which_all(small);
    which_all.insert(which_all.end(), big.begin(), big.end());
    int small_N = 1, big_N = 1;
    for (int p : small) small_N = std::max(small_N, prob[p].N);
    for (int p : big) big_N = std::max(big_N, prob[p].N);

    SK_AUC_HIP(hipSetDevice(sk::ctx_device(ctx)));
    // a fresh timing set for the launch events below, collected before this
    // call returns (as sk_svm_train_batch does): the call is synchronous
    SK_AUC_HIP(sk::call_begin(ctx));
    hipStream_t S = sk::ctx_stream(ctx);
    size_t off = 0;
    auto take = [&](size_t bytes) {
      const size_t at = off;
      off += (bytes + 255) & ~(size_t)255;
      return at;
    };
    const size_t nn8 = (size_t)n * n * 8;
    const size_t o_gram = take(nn8), o_grads = take(nn8 * n_params), o_y = take((size_t)n),
                 o_tr = take((size_t)sum_train * 4), o_ts = take((size_t)sum_test * 4),
                 o_al = take((size_t)sum_train * 8), o_de = take((size_t)sum_test * 8),
                 o_pr = take((size_t)n_problems * sizeof(sk::AucProb)), o_wh = take((size_t)n_problems * 4),
                 o_uty = take((size_t)sum_list * 4), o_uk = take((size_t)sum_list * 4),
                 o_cty = take((size_t)sum_list * 4), o_cg = take((size_t)n_problems * 8),
                 o_fg = take((size_t)n_problems * n_params * 8), o_du = take((size_t)sum_du * 8),
                 o_in = take((size_t)n_problems * sizeof(sk_auc_info)), o_sc = take((size_t)scratch_max * 8);
    sk::DevBuf buf;
    if (hipMalloc(&buf.p, off) != hipSuccess) {
      (void)hipGetLastError();
      return sk::ctx_fail(ctx, SK_ERR_ALLOC, "sk_auc_gradient_batch: device memory for the matrices and the scratch");
    }
    char* base = static_cast<char*>(buf.p);
    auto up = [&](size_t at, const void* src, size_t bytes) {
      return bytes ? hipMemcpyAsync(base + at, src, bytes, hipMemcpyHostToDevice, S) : hipSuccess;
    };
    SK_AUC_HIP(up(o_gram, gram, nn8));
    SK_AUC_HIP(up(o_grads, grads, nn8 * n_params));
    SK_AUC_HIP(up(o_y, ypos.data(), (size_t)n));
    SK_AUC_HIP(up(o_tr, train.data(), (size_t)sum_train * 4));
    SK_AUC_HIP(up(o_ts, test.data(), (size_t)sum_test * 4));
    SK_AUC_HIP(up(o_al, alpha.data(), (size_t)sum_train * 8));
    SK_AUC_HIP(up(o_de, delta.data(), (size_t)sum_test * 8));
    SK_AUC_HIP(up(o_pr, prob.data(), (size_t)n_problems * sizeof(sk::AucProb)));
    SK_AUC_HIP(up(o_wh, which_all.data(), (size_t)n_problems * 4));
    SK_AUC_HIP(hipMemsetAsync(base + o_du, 0, (size_t)sum_du * 8, S));
    sk::AucLaunch L;
    L.gram = reinterpret_cast<const double*>(base + o_gram);
    L.grads = reinterpret_cast<const double*>(base + o_grads);
    L.n_params = n_params, L.n = n;
    L.ypos = reinterpret_cast<const signed char*>(base + o_y);
    L.train = reinterpret_cast<const int32_t*>(base + o_tr);
    L.test = reinterpret_cast<const int32_t*>(base + o_ts);
    L.alpha = reinterpret_cast<const double*>(base + o_al);
    L.delta = reinterpret_cast<const double*>(base + o_de);
    L.prob = reinterpret_cast<const sk::AucProb*>(base + o_pr);
    L.u_ty = reinterpret_cast<int32_t*>(base + o_uty);
    L.u_k = reinterpret_cast<int32_t*>(base + o_uk);
    L.c_ty = reinterpret_cast<int32_t*>(base + o_cty);
    L.scratch = reinterpret_cast<double*>(base + o_sc);
    L.cg = reinterpret_cast<double*>(base + o_cg);
    L.fg = reinterpret_cast<double*>(base + o_fg);
    L.du = reinterpret_cast<double*>(base + o_du);
    L.info = reinterpret_cast<sk_auc_info*>(base + o_in);
    const int32_t* which_dev = reinterpret_cast<const int32_t*>(base + o_wh);

    // the scratch class first: its workgroups run longest
    if (!big.empty()) {
      auto fn = sk::sk_auc_grad_kernel<sk::kAucThreadsScratch, false>;
      const size_t lds = sk::lds_bytes(big_N, false);
      SK_AUC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
      for (const auto& wv : waves) {
        L.which = which_dev + small.size() + wv.first;
        SK_AUC_HIP(sk::lev_mark(ctx, S));
        hipLaunchKernelGGL(fn, dim3(wv.second - wv.first), dim3(sk::kAucThreadsScratch), lds, S, L);
        SK_AUC_HIP(hipGetLastError());
        SK_AUC_HIP(sk::lev_mark(ctx, S));
      }
    }
    if (!small.empty()) {
      auto fn = sk::sk_auc_grad_kernel<sk::kAucThreadsLds, true>;
      const size_t lds = sk::lds_bytes(small_N, true);
      SK_AUC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
      L.which = which_dev;
      SK_AUC_HIP(sk::lev_mark(ctx, S));
      hipLaunchKernelGGL(fn, dim3((int)small.size()), dim3(sk::kAucThreadsLds), lds, S, L);
      SK_AUC_HIP(hipGetLastError());
      SK_AUC_HIP(sk::lev_mark(ctx, S));
    }
    std::vector<double> du_host((size_t)sum_du);  // always read back: finite looks at d_u
    SK_AUC_HIP(hipMemcpyAsync(cg_out, base + o_cg, (size_t)n_problems * 8, hipMemcpyDeviceToHost, S));
    if (n_params)
      SK_AUC_HIP(hipMemcpyAsync(fg_out, base + o_fg, (size_t)n_problems * n_params * 8, hipMemcpyDeviceToHost, S));
    SK_AUC_HIP(hipMemcpyAsync(du_host.data(), base + o_du, (size_t)sum_du * 8, hipMemcpyDeviceToHost, S));
    SK_AUC_HIP(hipMemcpyAsync(info, base + o_in, (size_t)n_problems * sizeof(sk_auc_info), hipMemcpyDeviceToHost, S));
    SK_AUC_HIP(hipStreamSynchronize(S));
    SK_AUC_HIP(sk::lev_collect(ctx));
    for (int p = 0; p < n_problems; ++p) {
      if (info[p].n_free != nf[p] || info[p].n_bound != nb[p])
        return sk::ctx_fail(ctx, SK_ERR_HIP, "sk_auc_gradient_batch: the kernel's support-vector counts are not the host's");
      const int n_du = nf[p] > 0 ? nf[p] + 1 : 0;
      info[p].finite = sk::auc_outputs_finite(cg_out[p], fg_out ? fg_out + (size_t)p * n_params : nullptr, n_params,
                                              du_host.data() + du_off[p], n_du);
      if (d_u_out && n_du) std::memcpy(d_u_out + du_off[p], du_host.data() + du_off[p], (size_t)n_du * 8);
    }
    return SK_OK;
  } catch (const std::bad_alloc&) {
    return sk::ctx_fail(ctx, SK_ERR_ALLOC, "sk_auc_gradient_batch: host memory");
  }
}
