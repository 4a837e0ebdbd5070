// Batched C-SVC training on CDNA4 (gfx950): libsvm's SMO solver without
// shrinking, one workgroup per (training subset, C) problem over one Gram
// resident in device memory.
//
// Reference: Solver::Solve  libsvm/solver.cpp:81-349, select_working_set
//   :352-451, calculate_rho :554-592, SVC_Q libsvm/qmatrix.cpp:339-362; the
//   arithmetic contract is the one csrc/host/svm_train.cpp restates (float Q
//   entries and quad_coef, double everything else, no fused multiply-add),
//   and the alphas are that file's bit for bit: every rounded operation below
//   is an explicit __d*_rn / __f*_rn, which the compiler does not contract.
//
// Schedule.  A workgroup of T threads (T = 64, 256 or 1,024: the size
// classes, kSvmElems elements per thread each, so n_train <= 256, 1,024 or
// 4,096) solves one problem.  Thread tid owns the training examples
// k = tid, tid + T, ...: their G and alpha (double), QD (float), label, Gram
// index and bound status stay in registers for the whole solve, and a row of
// the Gram is gathered with consecutive lanes on consecutive k.  One iteration:
//   1. every thread scans its elements for the maximiser of -y G over I_up;
//      a butterfly over the wave, then over the waves through LDS, combines
//      (value, index) pairs -- larger value, of equal values the larger index,
//      which is what a sequential scan with >= keeps.  The thread that owns
//      the wave's winner writes the wave's record with that element's alpha
//      and QD, so after one barrier every thread knows i, G_i, alpha_i, QD_i.
//   2. every thread reads its entries of row t_i, computes obj_diff for its
//      elements of I_low and Gmax2; the same combine with (smaller value,
//      larger index); the winner's owner adds G_j, alpha_j, QD_j.  Second
//      barrier.
//   3. the stopping test, then the two-variable update: computed by every
//      thread from the same values (uniform, so no broadcast and no third
//      barrier); the owners of i and j keep the new alphas and statuses.
//   4. every thread reads its entries of row t_j and updates its G.
// Two barriers and two dependent row gathers per iteration.  The Gram is read
// by row only (row t_i for Q_i), as the reference's kernel_precomputed does.
//
// After the solve: rho's sum over the free variables and obj's sum are added
// up in index order by one thread from LDS (so rho and obj are the host
// path's bits too; 2 x n_train dependent adds, microseconds); the bounds,
// n_free and n_bound by exact reductions.  Decision values of the test list:
// one wave per test example, lanes over the training examples, a butterfly
// sum -- the one place where the order of a sum differs from the host's.
//
// LDS per workgroup: 12 bytes per element slot (48 KiB in the largest class)
// and the waves' records.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../host/runtime.h"
#include "../host/svm_train.h"

namespace sk {

namespace {

struct SvmProb {
  int64_t max_iter;
  double Cp, Cn, eps;
  int32_t train_off, n_train, test_off, n_test;
};
struct SvmLaunch {
  const double* gram;
  int32_t n;
  const signed char* ypos;  // per example of the Gram: 1 when its label is > 0
  const int32_t* train;     // the problems' training lists, concatenated
  const int32_t* test;
  const SvmProb* prob;
  const int32_t* which;     // the problems of this launch's class
  double* alpha;
  double* dec;
  sk_svm_solution* sol;
};

struct RecI {  // a wave's candidate for i
  double v, alpha;
  float qd;
  int32_t idx;
};
struct RecJ {  // a wave's candidate for j
  double od, g, alpha;
  float qd;
  int32_t idx;
};

constexpr double kSvmTau = 1e-12;
enum : int { kStLower = 0, kStUpper = 1, kStFree = 2, kStAbsent = 3 };

__device__ __forceinline__ double shfl_xor_f64(double v, int m) { return __shfl_xor(v, m, 64); }

template <int T>
__global__ void __launch_bounds__(T) sk_svm_smo_kernel(SvmLaunch L) {
  constexpr int E = kSvmElems, W = T / 64, CAP = T * E;
  __shared__ double s_val[CAP];
  __shared__ int32_t s_ty[CAP];  // (Gram index << 1) | (y > 0)
  __shared__ RecI s_ri[W];
  __shared__ RecJ s_rj[W];
  __shared__ double s_g2[W];
  __shared__ double s_ub[W], s_lb[W];
  __shared__ int32_t s_nf[W], s_nb[W];
  __shared__ double s_seq[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SvmProb P = L.prob[L.which[blockIdx.x]];
  const int l = P.n_train;
  const size_t n = (size_t)L.n;
  const double* __restrict__ K = L.gram;
  const int32_t* __restrict__ tr = L.train + P.train_off;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);

  int tk[E], yk[E], st[E];
  float qd[E], qi[E], qj[E];
  double G[E], al[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int k = e * T + tid;
    tk[e] = 0, yk[e] = 1, st[e] = kStAbsent, qd[e] = 0.f, qi[e] = 0.f, qj[e] = 0.f, G[e] = 0.0, al[e] = 0.0;
    if (k < l) {
      const int t = tr[k];
      tk[e] = t;
      yk[e] = L.ypos[t] ? 1 : -1;
      st[e] = kStLower;
      qd[e] = (float)K[(size_t)t * n + t];
      G[e] = -1.0;
      s_ty[k] = (t << 1) | (yk[e] > 0 ? 1 : 0);
    }
  }
  __syncthreads();

  int64_t iter = 0;
  int status = SK_SVM_CONVERGED;
  for (;;) {
    // ---- 1. i: the last maximiser of -y G over I_up
    double v = -inf;
    int idx = -1;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (st[e] == kStAbsent) continue;
      const int k = e * T + tid;
      if (yk[e] > 0) {
        if (st[e] != kStUpper && -G[e] >= v) v = -G[e], idx = k;
      } else {
        if (st[e] != kStLower && G[e] >= v) v = G[e], idx = k;
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double ov = shfl_xor_f64(v, m);
      const int oi = __shfl_xor(idx, m, 64);
      if (ov > v || (ov == v && oi > idx)) v = ov, idx = oi;
    }
    if (idx >= 0 ? (idx & (T - 1)) == tid : lane == 0) {
      const int slot = idx >= 0 ? idx / T : 0;
      RecI r;
      r.v = v, r.idx = idx, r.alpha = 0.0, r.qd = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (e == slot) r.alpha = al[e], r.qd = qd[e];
      s_ri[wave] = r;
    }
    __syncthreads();
    double gmax = -inf, ai0 = 0.0;
    float qd_i = 0.f;
    int i = -1;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const RecI r = s_ri[w];
      if (r.v > gmax || (r.v == gmax && r.idx > i)) gmax = r.v, i = r.idx, ai0 = r.alpha, qd_i = r.qd;
    }
    int y_i = 1;
    const double* __restrict__ ri = K;
    if (i >= 0) {
      const int ty = s_ty[i];
      y_i = (ty & 1) ? 1 : -1;
      ri = K + (size_t)(ty >> 1) * n;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (st[e] != kStAbsent) qi[e] = (float)((double)(y_i * yk[e]) * ri[tk[e]]);
    }

    // ---- 2. j: the last minimiser of the objective's decrease over I_low
    double od = inf, g2 = -inf;
    int jdx = -1;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (st[e] == kStAbsent) continue;
      double gd;
      float qf;
      if (yk[e] > 0) {
        if (st[e] == kStLower) continue;
        gd = __dadd_rn(gmax, G[e]);
        if (G[e] >= g2) g2 = G[e];
        if (!(gd > 0)) continue;
        qf = __fsub_rn(__fadd_rn(qd_i, qd[e]), __fmul_rn((float)(2 * y_i), qi[e]));
      } else {
        if (st[e] == kStUpper) continue;
        gd = __dsub_rn(gmax, G[e]);
        if (-G[e] >= g2) g2 = -G[e];
        if (!(gd > 0)) continue;
        qf = __fadd_rn(__fadd_rn(qd_i, qd[e]), __fmul_rn((float)(2 * y_i), qi[e]));
      }
      const double qc = (double)qf;
      const double od_e = -__ddiv_rn(__dmul_rn(gd, gd), qc > 0 ? qc : kSvmTau);
      if (od_e <= od) od = od_e, jdx = e * T + tid;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double oo = shfl_xor_f64(od, m);
      const int oj = __shfl_xor(jdx, m, 64);
      const double og = shfl_xor_f64(g2, m);
      if (oo < od || (oo == od && oj > jdx)) od = oo, jdx = oj;
      if (og > g2) g2 = og;
    }
    if (jdx >= 0 ? (jdx & (T - 1)) == tid : lane == 0) {
      const int slot = jdx >= 0 ? jdx / T : 0;
      RecJ r;
      r.od = od, r.idx = jdx, r.g = 0.0, r.alpha = 0.0, r.qd = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (e == slot) r.g = G[e], r.alpha = al[e], r.qd = qd[e];
      s_rj[wave] = r;
    }
    if (lane == 0) s_g2[wave] = g2;
    __syncthreads();
    double od_min = inf, gmax2 = -inf, G_j = 0.0, aj0 = 0.0;
    float qd_j = 0.f;
    int j = -1;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const RecJ r = s_rj[w];
      if (r.od < od_min || (r.od == od_min && r.idx > j))
        od_min = r.od, j = r.idx, G_j = r.g, aj0 = r.alpha, qd_j = r.qd;
      const double g = s_g2[w];
      if (g > gmax2) gmax2 = g;
    }

    // ---- 3. stop, or update alpha_i and alpha_j (every thread, same values)
    if (__dadd_rn(gmax, gmax2) < P.eps) break;
    if (i < 0 || j < 0) {
      status = SK_SVM_NO_PAIR;
      break;
    }
    if (iter == P.max_iter) {
      status = SK_SVM_NOT_CONVERGED;
      break;
    }
    ++iter;
    const int tyj = s_ty[j];
    const int y_j = (tyj & 1) ? 1 : -1;
    const double* __restrict__ rj = K + (size_t)(tyj >> 1) * n;
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (st[e] != kStAbsent) qj[e] = (float)((double)(y_j * yk[e]) * rj[tk[e]]);
    const float q_ij = (float)((double)(y_i * y_j) * ri[tyj >> 1]);
    const double G_i = y_i > 0 ? -gmax : gmax;
    const double Ci = y_i > 0 ? P.Cp : P.Cn, Cj = y_j > 0 ? P.Cp : P.Cn;
    double ai = ai0, aj = aj0;
    if (y_i != y_j) {
      const float qf = __fadd_rn(__fadd_rn(qd_i, qd_j), __fmul_rn(2.f, q_ij));
      double qc = (double)qf;
      if (qc <= 0) qc = kSvmTau;
      const double delta = __ddiv_rn(__dsub_rn(-G_i, G_j), qc);
      const double diff = __dsub_rn(ai, aj);
      ai = __dadd_rn(ai, delta);
      aj = __dadd_rn(aj, delta);
      if (diff > 0) {
        if (aj < 0) aj = 0, ai = diff;
      } else {
        if (ai < 0) ai = 0, aj = -diff;
      }
      if (diff > __dsub_rn(Ci, Cj)) {
        if (ai > Ci) ai = Ci, aj = __dsub_rn(Ci, diff);
      } else {
        if (aj > Cj) aj = Cj, ai = __dadd_rn(Cj, diff);
      }
    } else {
      const float qf = __fsub_rn(__fadd_rn(qd_i, qd_j), __fmul_rn(2.f, q_ij));
      double qc = (double)qf;
      if (qc <= 0) qc = kSvmTau;
      const double delta = __ddiv_rn(__dsub_rn(G_i, G_j), qc);
      const double sum = __dadd_rn(ai, aj);
      ai = __dsub_rn(ai, delta);
      aj = __dadd_rn(aj, delta);
      if (sum > Ci) {
        if (ai > Ci) ai = Ci, aj = __dsub_rn(sum, Ci);
      } else {
        if (aj < 0) aj = 0, ai = sum;
      }
      if (sum > Cj) {
        if (aj > Cj) aj = Cj, ai = __dsub_rn(sum, Cj);
      } else {
        if (ai < 0) ai = 0, aj = sum;
      }
    }
    const double dai = __dsub_rn(ai, ai0), daj = __dsub_rn(aj, aj0);

    // ---- 4. G, and the owners' alphas
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (st[e] != kStAbsent)
        G[e] = __dadd_rn(G[e], __dadd_rn(__dmul_rn((double)qi[e], dai), __dmul_rn((double)qj[e], daj)));
    if ((i & (T - 1)) == tid) {
      const int slot = i / T;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (e == slot) al[e] = ai, st[e] = ai >= Ci ? kStUpper : ai <= 0 ? kStLower : kStFree;
    }
    if ((j & (T - 1)) == tid) {
      const int slot = j / T;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (e == slot) al[e] = aj, st[e] = aj >= Cj ? kStUpper : aj <= 0 ? kStLower : kStFree;
    }
  }

  // ---- rho: the free variables' y G summed in index order (adding +0.0 for
  // the others changes no bit: the sum starts at +0.0); bounds by reduction
  double ub = inf, lb = -inf;
  int nf = 0, nb = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if (st[e] == kStAbsent) continue;
    const double yg = yk[e] > 0 ? G[e] : -G[e];
    double f = 0.0;
    if (st[e] == kStUpper) {
      ++nb;
      if (yk[e] < 0) ub = yg < ub ? yg : ub;
      else lb = yg > lb ? yg : lb;
    } else if (st[e] == kStLower) {
      if (yk[e] > 0) ub = yg < ub ? yg : ub;
      else lb = yg > lb ? yg : lb;
    } else {
      ++nf;
      f = yg;
    }
    s_val[e * T + tid] = f;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double ou = shfl_xor_f64(ub, m), ol = shfl_xor_f64(lb, m);
    ub = ou < ub ? ou : ub;
    lb = ol > lb ? ol : lb;
    nf += __shfl_xor(nf, m, 64);
    nb += __shfl_xor(nb, m, 64);
  }
  if (lane == 0) s_ub[wave] = ub, s_lb[wave] = lb, s_nf[wave] = nf, s_nb[wave] = nb;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int k = 0; k < l; ++k) sum = __dadd_rn(sum, s_val[k]);
    s_seq[0] = sum;
  }
  ub = inf, lb = -inf, nf = 0, nb = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    ub = s_ub[w] < ub ? s_ub[w] : ub;
    lb = s_lb[w] > lb ? s_lb[w] : lb;
    nf += s_nf[w];
    nb += s_nb[w];
  }
  __syncthreads();
  const double rho = nf > 0 ? __ddiv_rn(s_seq[0], (double)nf) : __ddiv_rn(__dadd_rn(ub, lb), 2.0);
  // ---- obj = sum alpha (G + p) / 2, in index order
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (st[e] != kStAbsent) s_val[e * T + tid] = __dmul_rn(al[e], __dadd_rn(G[e], -1.0));
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int k = 0; k < l; ++k) sum = __dadd_rn(sum, s_val[k]);
    sk_svm_solution S;
    S.rho = rho;
    S.obj = __ddiv_rn(sum, 2.0);
    S.iterations = iter;
    S.status = status;
    S.n_free = nf;
    S.n_bound = nb;
    L.sol[L.which[blockIdx.x]] = S;
  }
  __syncthreads();
  // ---- alphas out; decision values of the test list
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (st[e] != kStAbsent) {
      const int k = e * T + tid;
      L.alpha[P.train_off + k] = al[e];
      s_val[k] = yk[e] > 0 ? al[e] : -al[e];
    }
  __syncthreads();
  for (int q = wave; q < P.n_test; q += W) {
    const double* __restrict__ rs = K + (size_t)L.test[P.test_off + q] * n;
    double sum = 0.0;
    for (int a = lane; a < l; a += 64) {
      const double c = s_val[a];
      if (c != 0.0) sum = __dadd_rn(sum, __dmul_rn(c, rs[s_ty[a] >> 1]));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum = __dadd_rn(sum, shfl_xor_f64(sum, m));
    if (lane == 0) L.dec[P.test_off + q] = __dsub_rn(sum, rho);
  }
}

template <int T>
hipError_t launch_class(const SvmLaunch& L, int grid, hipStream_t st) {
  hipLaunchKernelGGL(sk_svm_smo_kernel<T>, dim3(grid), dim3(T), 0, st, L);
  return hipGetLastError();
}

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

}  // namespace
}  // namespace sk

#define SK_SVM_HIP(expr)                                                                                 \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess)                                                                                \
      return sk::ctx_fail(ctx, SK_ERR_HIP, std::string("sk_svm_train_batch: " #expr ": ") + hipGetErrorString(_e)); \
  } while (0)

extern "C" int sk_svm_train_batch(sk_context* ctx, const double* gram, int32_t n, const double* labels,
                                  const sk_svm_problem* problems, int32_t n_problems, double* alpha_out,
                                  double* dec_out, sk_svm_solution* solutions) {
  if (!ctx) return SK_ERR_INVALID;
  try {
    sk::lev_reset(ctx);
    std::string err;
    int64_t sum_train = 0, sum_test = 0;
    const int rc = sk::svm_check_batch(gram, n, labels, problems, n_problems, alpha_out, dec_out, solutions,
                                       sk::kSvmMaxTrain, &sum_train, &sum_test, err);
    if (rc) return sk::ctx_fail(ctx, rc, err);
    if (n_problems == 0) return SK_OK;
    if (sum_train > INT32_MAX || sum_test > INT32_MAX)
      return sk::ctx_fail(ctx, SK_ERR_UNSUPPORTED, "sk_svm_train_batch: over 2^31 list entries in one call");

    // host images: labels' signs, the lists concatenated, the descriptors, the classes' problems
    std::vector<signed char> ypos(n);
    for (int32_t k = 0; k < n; ++k) ypos[k] = labels[k] > 0 ? 1 : 0;
    std::vector<int32_t> train((size_t)sum_train), test((size_t)sum_test);
    std::vector<sk::SvmProb> prob(n_problems);
    std::vector<int32_t> which[sk::kSvmClasses];
    int32_t to = 0, so = 0;
    for (int p = 0; p < n_problems; ++p) {
      const sk_svm_problem& P = problems[p];
      sk::SvmProb& D = prob[p];
      D.max_iter = P.max_iter;
      D.Cp = P.Cp, D.Cn = P.Cn, D.eps = P.eps;
      D.train_off = to, D.n_train = P.n_train, D.test_off = so, D.n_test = P.n_test;
      std::memcpy(train.data() + to, P.train, (size_t)P.n_train * 4);
      if (P.n_test) std::memcpy(test.data() + so, P.test, (size_t)P.n_test * 4);
      to += P.n_train;
      so += P.n_test;
      int c = 0;
      while (P.n_train > sk::kSvmThreads[c] * sk::kSvmElems) ++c;
      which[c].push_back(p);
    }
    std::vector<int32_t> which_all;
    int32_t which_off[sk::kSvmClasses];
    for (int c = 0; c < sk::kSvmClasses; ++c) {
      which_off[c] = (int32_t)which_all.size();
      which_all.insert(which_all.end(), which[c].begin(), which[c].end());
    }

    SK_SVM_HIP(hipSetDevice(sk::ctx_device(ctx)));
    // a fresh timing set for the launch events below, collected before this
    // call returns (lev_collect), so no call_finish: the call is synchronous and
    // stages nothing.  On an asynchronous context call_begin also advances the
    // staging ring by one slot, which this call leaves empty (sk_bpla_gradients
    // does the same).
    SK_SVM_HIP(sk::call_begin(ctx));
    hipStream_t S = sk::ctx_stream(ctx);
    // one device arena
    size_t off = 0;
    auto take = [&](size_t bytes) {
      const size_t at = off;
      off += (bytes + 255) & ~(size_t)255;
      return at;
    };
    const size_t o_gram = take((size_t)n * n * 8), o_y = take((size_t)n), o_tr = take((size_t)sum_train * 4),
                 o_ts = take((size_t)sum_test * 4), o_pr = take((size_t)n_problems * sizeof(sk::SvmProb)),
                 o_wh = take((size_t)n_problems * 4), o_al = take((size_t)sum_train * 8),
                 o_de = take((size_t)sum_test * 8), o_so = take((size_t)n_problems * sizeof(sk_svm_solution));
    sk::DevBuf buf;
    if (hipMalloc(&buf.p, off) != hipSuccess) {
      (void)hipGetLastError();
      return sk::ctx_fail(ctx, SK_ERR_ALLOC, "sk_svm_train_batch: device memory for the Gram and the lists");
    }
    char* base = static_cast<char*>(buf.p);
    auto up = [&](size_t at, const void* src, size_t bytes) {
      return bytes ? hipMemcpyAsync(base + at, src, bytes, hipMemcpyHostToDevice, S) : hipSuccess;
    };
    SK_SVM_HIP(up(o_gram, gram, (size_t)n * n * 8));
    SK_SVM_HIP(up(o_y, ypos.data(), (size_t)n));
    SK_SVM_HIP(up(o_tr, train.data(), (size_t)sum_train * 4));
    SK_SVM_HIP(up(o_ts, test.data(), (size_t)sum_test * 4));
    SK_SVM_HIP(up(o_pr, prob.data(), (size_t)n_problems * sizeof(sk::SvmProb)));
    SK_SVM_HIP(up(o_wh, which_all.data(), (size_t)n_problems * 4));
    sk::SvmLaunch L;
    L.gram = reinterpret_cast<const double*>(base + o_gram);
    L.n = n;
    L.ypos = reinterpret_cast<const signed char*>(base + o_y);
    L.train = reinterpret_cast<const int32_t*>(base + o_tr);
    L.test = reinterpret_cast<const int32_t*>(base + o_ts);
    L.prob = reinterpret_cast<const sk::SvmProb*>(base + o_pr);
    L.alpha = reinterpret_cast<double*>(base + o_al);
    L.dec = reinterpret_cast<double*>(base + o_de);
    L.sol = reinterpret_cast<sk_svm_solution*>(base + o_so);
    // largest class first: its workgroups run longest
    for (int c = sk::kSvmClasses - 1; c >= 0; --c) {
      if (which[c].empty()) continue;
      L.which = reinterpret_cast<const int32_t*>(base + o_wh) + which_off[c];
      const int grid = (int)which[c].size();
      SK_SVM_HIP(sk::lev_mark(ctx, S));
      if (c == 0) SK_SVM_HIP(sk::launch_class<sk::kSvmThreads[0]>(L, grid, S));
      if (c == 1) SK_SVM_HIP(sk::launch_class<sk::kSvmThreads[1]>(L, grid, S));
      if (c == 2) SK_SVM_HIP(sk::launch_class<sk::kSvmThreads[2]>(L, grid, S));
      SK_SVM_HIP(sk::lev_mark(ctx, S));
    }
    SK_SVM_HIP(hipMemcpyAsync(alpha_out, base + o_al, (size_t)sum_train * 8, hipMemcpyDeviceToHost, S));
    if (sum_test)
      SK_SVM_HIP(hipMemcpyAsync(dec_out, base + o_de, (size_t)sum_test * 8, hipMemcpyDeviceToHost, S));
    SK_SVM_HIP(hipMemcpyAsync(solutions, base + o_so, (size_t)n_problems * sizeof(sk_svm_solution),
                              hipMemcpyDeviceToHost, S));
    SK_SVM_HIP(hipStreamSynchronize(S));
    SK_SVM_HIP(sk::lev_collect(ctx));
    return SK_OK;
  } catch (const std::bad_alloc&) {
    return sk::ctx_fail(ctx, SK_ERR_ALLOC, "sk_svm_train_batch: host memory");
  }
}
