// The optimizer's cross-validated AUC gradient, restated from the reference
// with the association of every product and the ascending order of every sum:
//   GradientComputation::compute       optimizer/gradient.cpp:107-156 (steps 3-5)
//   GradientComputationAUC::compute_delta  gradient.cpp:159-206
//   sigmoid, sign, calculate_avg_var   gradient.cpp:336-366
//   find_support_vectors               gradient.cpp:368-403
//   solve_d                            gradient.cpp:405-456
//   calculate_gradient_c               gradient.cpp:511-547
//   calculate_gradient_p               gradient.cpp:549-620
//   conjugate_gradient                 gradient.cpp:622-644
// The reference's vectors and matrices are uBLAS's: prod(A, v)(i) and
// inner_prod(a, b) start at zero and add their terms in ascending index, and
// an expression such as q - prod(A, v) is evaluated element by element.
//
// The KKT system of solve_d is indefinite and the reference's conjugate
// gradient on it amplifies rounding, so nothing here may sum in
// another order: this file is the CPU path of sk_auc_gradient_batch, what
// tests/golden/auc_gradient.json pins, and what the GPU kernel
// (kernels/auc_grad.hip) is compared with, bit for bit.  Built with
// -ffp-contract=off.
#include "auc_gradient.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <system_error>
#include <thread>

namespace {

constexpr double kSigmoidConst = 10.0;  // SIGMOID_CONST, gradient.cpp:18
constexpr double kCgTol = 1e-10;

struct Dense {  // (nsv+1)^2, row-major
  int N;
  std::vector<double> a;
  double& operator()(int i, int j) { return a[(size_t)i * N + j]; }
  double operator()(int i, int j) const { return a[(size_t)i * N + j]; }
};

void prod(const Dense& A, const std::vector<double>& v, std::vector<double>& out) {
  const int N = A.N;
  for (int i = 0; i < N; ++i) {
    double t = 0.0;
    for (int j = 0; j < N; ++j) t += A(i, j) * v[j];
    out[i] = t;
  }
}

double inner(const std::vector<double>& a, const std::vector<double>& b) {
  double t = 0.0;
  for (size_t i = 0; i < a.size(); ++i) t += a[i] * b[i];
  return t;
}

// conjugate_gradient (gradient.cpp:622-644) from x = 0; returns the number of
// products A w it formed (0 on the early return)
int conjugate_gradient(const Dense& A, const std::vector<double>& b, std::vector<double>& x) {
  const int N = A.N;
  std::vector<double> r(N), w(N), z(N);
  prod(A, x, z);
  for (int i = 0; i < N; ++i) r[i] = b[i] - z[i];
  if (inner(r, r) < kCgTol) return 0;
  for (int i = 0; i < N; ++i) w[i] = -r[i];
  prod(A, w, z);
  int products = 1;
  double wz = inner(w, z);
  double a = inner(r, w) / wz;
  for (int i = 0; i < N; ++i) x[i] += a * w[i];
  for (int pass = 0; pass < N; ++pass) {
    for (int i = 0; i < N; ++i) r[i] -= a * z[i];
    if (inner(r, r) < kCgTol) break;
    const double B = inner(r, z) / wz;  // w and z are the ones wz was formed from
    for (int i = 0; i < N; ++i) w[i] = -r[i] + B * w[i];
    prod(A, w, z);
    ++products;
    wz = inner(w, z);
    a = inner(r, w) / wz;
    for (int i = 0; i < N; ++i) x[i] += a * w[i];
  }
  return products;
}

void gradient_one(const double* K, const double* G, int32_t n_params, int32_t n, const double* labels,
                  const sk_auc_problem& P, double* cg_out, double* fg_out, double* d_out, sk_auc_info& info) {
  const size_t nn = (size_t)n;
  const int l = P.n_train, m = P.n_test;
  const double C = P.C, b = P.rho;
  const double* delta = P.delta;
  auto ysign = [&](int32_t t) { return labels[t] > 0 ? +1 : -1; };

  // find_support_vectors
  std::vector<int32_t> u, c;
  std::vector<double> alpha_u;
  for (int k = 0; k < l; ++k) {
    if (0.0 < P.alpha[k] && P.alpha[k] < C) u.push_back(P.train[k]), alpha_u.push_back(P.alpha[k]);
    else if (P.alpha[k] >= C) c.push_back(P.train[k]);
  }
  const int nsv = (int)u.size(), nc = (int)c.size(), N = nsv + 1;
  info.n_free = nsv;
  info.n_bound = nc;
  info.cg_iterations = 0;

  // solve_d
  std::vector<double> d_u;
  if (nsv > 0) {
    Dense p_u{N, std::vector<double>((size_t)N * N)};
    std::vector<double> r_u(N);
    for (int i = 0; i < nsv; ++i) {
      const int yi = ysign(u[i]);
      const double* row = K + (size_t)u[i] * nn;
      for (int j = 0; j < nsv; ++j) p_u(i, j) = (yi * ysign(u[j])) * row[u[j]];
      p_u(i, nsv) = p_u(nsv, i) = -yi;
      double t = 0.0;
      for (int j = 0; j < m; ++j) t += delta[j] * yi * row[P.test[j]];
      r_u[i] = t;
    }
    p_u(nsv, nsv) = 0.0;
    double t = 0.0;
    for (int j = 0; j < m; ++j) t -= delta[j];
    r_u[nsv] = t;
    d_u.assign(N, 0.0);
    info.cg_iterations = conjugate_gradient(p_u, r_u, d_u);
  }

  // calculate_gradient_c
  double cg = 0.0;
  std::vector<double> q(N), v(N);
  if (nsv > 0) {
    for (int i = 0; i < nsv; ++i) {
      const int yi = ysign(u[i]);
      const double* row = K + (size_t)u[i] * nn;
      double t = 0.0;
      for (int j = 0; j < nc; ++j) t -= (yi * ysign(c[j])) * row[c[j]];
      q[i] = t;
    }
    double t = 0.0;
    for (int j = 0; j < nc; ++j) t += ysign(c[j]);
    q[nsv] = t;
    cg += inner(d_u, q);
  }
  for (int i = 0; i < m; ++i) {
    const double* row = K + (size_t)P.test[i] * nn;
    for (int j = 0; j < nc; ++j) cg += delta[i] * ysign(c[j]) * row[c[j]];
  }
  *cg_out = cg;

  // calculate_gradient_p
  for (int p = 0; p < n_params; ++p) {
    const double* g = G + (size_t)p * nn * nn;
    double ret = 0.0;
    if (nsv > 0) {
      for (int i = 0; i < nsv; ++i) {
        const int yi = ysign(u[i]);
        const double* row = g + (size_t)u[i] * nn;
        double t = 0.0;
        for (int j = 0; j < nc; ++j) t -= (yi * ysign(c[j])) * row[c[j]] * C;
        q[i] = t;
        // row i of prod(p_u_dot, beta_u): the border column is 0, beta_u(nsv) = b
        double s = 0.0;
        for (int j = 0; j < nsv; ++j) s += ((yi * ysign(u[j])) * row[u[j]]) * alpha_u[j];
        s += 0.0 * b;
        v[i] = s;
      }
      q[nsv] = 0.0;
      double s = 0.0;
      for (int j = 0; j < nsv; ++j) s += 0.0 * alpha_u[j];
      s += 0.0 * b;
      v[nsv] = s;
      double t = 0.0;
      for (int i = 0; i < N; ++i) t += d_u[i] * (q[i] - v[i]);
      ret += t;
    }
    double t = 0.0;
    for (int j = 0; j < l; ++j) {
      const int yj = ysign(P.train[j]);
      double dpsi = 0.0;
      for (int i = 0; i < m; ++i) dpsi += delta[i] * yj * g[(size_t)P.test[i] * nn + P.train[j]];
      t += dpsi * P.alpha[j];
    }
    t += 0.0 * b;
    ret += t;
    fg_out[p] = ret;
  }
  if (d_out)
    for (int i = 0; i < (int)d_u.size(); ++i) d_out[i] = d_u[i];
  info.finite = sk::auc_outputs_finite(cg, fg_out, n_params, d_u.data(), (int32_t)d_u.size());
}

}  // namespace

namespace sk {

int32_t auc_outputs_finite(double cg, const double* fg, int32_t n_params, const double* d_u, int32_t n_du) {
  bool ok = std::isfinite(cg);
  for (int p = 0; p < n_params; ++p) ok = ok && std::isfinite(fg[p]);
  for (int i = 0; i < n_du; ++i) ok = ok && std::isfinite(d_u[i]);
  return ok ? 1 : 0;
}

int auc_check_batch(const double* gram, const double* grads, int32_t n_params, int32_t n, const double* labels,
                    const sk_auc_problem* problems, int32_t n_problems, const double* cg_out,
                    const double* fg_out, const sk_auc_info* info, int32_t max_n, std::vector<int32_t>& n_free,
                    std::vector<int32_t>& n_bound, std::string& err) {
  auto bad = [&](int p, const char* what) {
    err = "sk_auc_gradient_batch: problem " + std::to_string(p) + ": " + what;
    return (int)SK_ERR_INVALID;
  };
  if (!gram || !labels || n < 1 || n_params < 0 || (n_params && !grads) || n_problems < 0 ||
      (n_problems && (!problems || !cg_out || !info)) || (n_problems && n_params && !fg_out)) {
    err = "sk_auc_gradient_batch: null or empty argument, or n_params < 0";
    return SK_ERR_INVALID;
  }
  n_free.assign(n_problems, 0);
  n_bound.assign(n_problems, 0);
  for (int p = 0; p < n_problems; ++p) {
    const sk_auc_problem& P = problems[p];
    if (P.n_train < 2 || !P.train || !P.alpha) return bad(p, "n_train < 2");
    if (P.n_test < 1 || !P.test || !P.delta) return bad(p, "n_test < 1");
    if (!(P.C > 0)) return bad(p, "C <= 0");
    for (int k = 0; k < P.n_train; ++k) {
      const int32_t t = P.train[k];
      if (t < 0 || t >= n) return bad(p, "training index outside [0, n)");
      if (labels[t] == 0 || labels[t] != labels[t]) return bad(p, "a label that is 0 or not a number");
      const double a = P.alpha[k];
      if (!std::isfinite(a) || a < 0) return bad(p, "alpha negative or not finite");
      if (0.0 < a && a < P.C) ++n_free[p];
      else if (a >= P.C) ++n_bound[p];
    }
    for (int k = 0; k < P.n_test; ++k) {
      const int32_t t = P.test[k];
      if (t < 0 || t >= n) return bad(p, "test index outside [0, n)");
      if (labels[t] == 0 || labels[t] != labels[t]) return bad(p, "a label that is 0 or not a number");
      if (!std::isfinite(P.delta[k])) return bad(p, "delta not finite");
    }
  }
  if (max_n > 0)
    for (int p = 0; p < n_problems; ++p)
      if (n_free[p] + 1 > max_n) {
        err = "sk_auc_gradient_batch: problem " + std::to_string(p) + ": " + std::to_string(n_free[p]) +
              " free support vectors; the GPU path's P scratch takes " + std::to_string(max_n - 1);
        return SK_ERR_UNSUPPORTED;
      }
  return SK_OK;
}

}  // namespace sk

extern "C" {

int sk_auc_delta(const double* dec, const double* labels_of_test, int32_t n_test, double* delta_out,
                 double* f_out) {
  if (n_test < 0 || (n_test && (!dec || !labels_of_test || !delta_out)) || !f_out) return SK_ERR_INVALID;
  try {
    // the differences, positives outer and negatives inner; a label >= 0 is positive
    std::vector<double> d;
    for (int i = 0; i < n_test; ++i)
      if (labels_of_test[i] >= 0)
        for (int j = 0; j < n_test; ++j)
          if (labels_of_test[j] < 0) d.push_back(dec[i] - dec[j]);
    for (int i = 0; i < n_test; ++i) delta_out[i] = 0.0;
    *f_out = 0.0;
    if (d.empty()) return SK_OK;  // one class: the reference's loops do not run
    const size_t m = d.size();
    double sum = 0.0, sum2 = 0.0;
    for (double x : d) {
      sum += x;
      sum2 += x * x;
    }
    const unsigned int mu = (unsigned int)m;  // calculate_avg_var's uint n
    const double avg = sum / mu;
    double var = sum2 / mu - avg * avg;
    if (var < 0.0) var = 0.0;
    if (var < 1e-10) var = 1e-10;
    const double rho = std::sqrt(var);
    const double s = kSigmoidConst / rho;
    const double s2 = -kSigmoidConst / (m * rho * var);
    double auc = 0.0;
    size_t v = 0;
    for (int i = 0; i < n_test; ++i)
      if (labels_of_test[i] >= 0)
        for (int j = 0; j < n_test; ++j)
          if (labels_of_test[j] < 0) {
            const double x = d[v++];
            const double sig = 1.0 / (1.0 + std::exp(-s * x));
            auc += sig / m;
            const double w = sig * (1.0 - sig) * (s + x * s2 * (x - avg)) / m;
            delta_out[i] += w;
            delta_out[j] -= w;
          }
    *f_out = auc;
    return SK_OK;
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
}

int sk_auc_gradient_batch_host(const double* gram, const double* grads, int32_t n_params, int32_t n,
                               const double* labels, const sk_auc_problem* problems, int32_t n_problems,
                               int32_t n_threads, double* cg_out, double* fg_out, double* d_u_out,
                               sk_auc_info* info) {
  try {
    std::string err;
    std::vector<int32_t> nf, nb;
    const int rc = sk::auc_check_batch(gram, grads, n_params, n, labels, problems, n_problems, cg_out, fg_out,
                                       info, 0, nf, nb, err);
    if (rc) return rc;
    if (n_threads < 0) return SK_ERR_INVALID;
    std::vector<int64_t> doff(n_problems + 1, 0);
    for (int p = 0; p < n_problems; ++p) doff[p + 1] = doff[p] + problems[p].n_train + 1;
    int nt = n_threads ? n_threads : (int)std::max(1u, std::thread::hardware_concurrency());
    nt = std::max(1, std::min(nt, n_problems));
    std::atomic<int> cursor{0};
    std::atomic<bool> oom{false};
    auto work = [&] {
      for (int p; (p = cursor.fetch_add(1)) < n_problems;) {
        try {
          gradient_one(gram, grads, n_params, n, labels, problems[p], cg_out + p,
                       fg_out ? fg_out + (size_t)p * n_params : nullptr, d_u_out ? d_u_out + doff[p] : nullptr,
                       info[p]);
        } catch (const std::bad_alloc&) {
          oom = true;
        }
      }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) {
      try {
        th.emplace_back(work);
      } catch (const std::system_error&) {
        break;  // the calling thread's share drains the cursor
      }
    }
    work();
    for (auto& x : th) x.join();
    return oom ? SK_ERR_ALLOC : SK_OK;
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
}

int sk_auc_gradient_shape(int32_t* lds_free, int32_t* max_free, int64_t* scratch_budget) {
  if (lds_free) *lds_free = sk::kAucLdsN - 1;
  if (max_free) *max_free = sk::kAucMaxN - 1;
  if (scratch_budget) *scratch_budget = sk::kAucScratchBudget;
  return SK_OK;
}

}  // extern "C"
