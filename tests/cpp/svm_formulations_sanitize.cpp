// Host code under a sanitizer: calls sk_svm_solve_batch_host on one task per
// svm_type (and a batch of all five on several threads) as a stand-alone
// program.  tests/test_svm_formulations_cpu.py compiles it together with
// stem_kernel_amd/csrc/host/svm_train.cpp with -fsanitize=address,undefined
// and runs it; the 2 l positions of the SVR types index every per-position
// array of the solver, which is where an off-by-l would hide.  Every buffer
// is allocated at its exact size, so a write past n_train coefficients or
// n_test decision values is a heap overflow the sanitizer reports.  It also
// runs C-SVC through sk_svm_train_batch_host_ex with shrinking off and on
// (c_svc_with_and_without_shrinking below).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "stem_kernel.h"

namespace {

uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// C-SVC through sk_svm_train_batch_host_ex, shrinking off and on: the same
// solver, which with shrinking swaps the entries of every per-position array,
// reads rows over the inactive tail and rebuilds the gradient there.  One
// integer Gram (K = A A^T / 4, n = 48, d = 3) with a permuted training list and
// Cp != Cn: a problem that shrinks, runs the unshrink branch and regrows its
// active set; the same stopped by max_iter between two shrink calls; and a
// shorter list.  Prints what it saw (the test asserts the counts) and returns
// the number of failures.
int c_svc_with_and_without_shrinking() {
  const int n = 48, d = 3;
  uint64_t s = 0x5A17E10E;
  std::vector<int> A((size_t)n * d);
  for (int& a : A) a = (int)(splitmix64(s) % 7) - 3;
  std::vector<double> K((size_t)n * n), y(n);
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) {
      long v = 0;
      for (int k = 0; k < d; ++k) v += (long)A[r * d + k] * A[c * d + k];
      K[(size_t)r * n + c] = std::ldexp((double)v, -2);
    }
  for (int r = 0; r < n; ++r) y[r] = (splitmix64(s) & 1) ? 1.0 : -1.0;
  y[0] = 1.0, y[1] = -1.0;
  std::vector<int32_t> train, test;
  for (int k = 0; k < n; ++k) train.push_back((k * 37 + 5) % n);
  for (int k = 0; k < n; k += 5) test.push_back(n - 1 - k);
  const sk_svm_problem problems[3] = {
      {train.data(), n, test.data(), (int32_t)test.size(), 16.0, 8.0, 1e-3, 1000000},
      {train.data(), n, test.data(), (int32_t)test.size(), 16.0, 8.0, 1e-3, 100},
      {train.data(), 30, nullptr, 0, 1.0, 0.25, 1e-3, 1000000},
  };
  int failures = 0, capped = 0, shrunk = 0, regrown = 0;
  for (int shrinking = 0; shrinking < 2; ++shrinking) {
    std::vector<double> alpha(n + n + 30), dec(2 * test.size());
    sk_svm_solution sol[3];
    sk_svm_shrink_info info[3];
    const int rc = sk_svm_train_batch_host_ex(K.data(), n, y.data(), problems, 3, 2, shrinking, alpha.data(), dec.data(),
                                              sol, info);
    if (rc != SK_OK) return failures + 1;
    const double* a = alpha.data();
    for (int p = 0; p < 3; ++p) {
      const sk_svm_problem& P = problems[p];
      const sk_svm_shrink_info& I = info[p];
      std::printf("c_svc problem %d shrinking %d: status %d iterations %lld rho %.6g obj %.6g shrink_calls %d "
                  "shrunk_calls %d min_active %d unshrunk %d regrown %d reconstructions %d resumed %d\n",
                  p, shrinking, sol[p].status, (long long)sol[p].iterations, sol[p].rho, sol[p].obj, I.shrink_calls,
                  I.shrunk_calls, I.min_active, I.unshrunk, I.regrown, I.reconstructions, I.resumed);
      for (int k = 0; k < P.n_train; ++k)
        if (!(a[k] >= 0 && a[k] <= (y[P.train[k]] > 0 ? P.Cp : P.Cn))) {
          ++failures;
          break;
        }
      a += P.n_train;
      if (sol[p].status != (P.max_iter == 100 ? SK_SVM_NOT_CONVERGED : SK_SVM_CONVERGED) || !std::isfinite(sol[p].rho))
        ++failures;
      if (!shrinking && (I.shrink_calls || I.shrunk_calls || I.min_active != P.n_train || I.unshrunk || I.regrown ||
                         I.reconstructions || I.resumed))
        ++failures;
      capped += sol[p].status == SK_SVM_NOT_CONVERGED;
      shrunk += I.shrunk_calls > 0;
      regrown += I.unshrunk == 1 && I.regrown == 1;
    }
  }
  std::printf("c_svc: capped %d shrunk %d regrown %d\n", capped, shrunk, regrown);
  return failures;
}

}  // namespace

int main() {
  // K = A A^T / 4 with small integers; labels +-1 with both classes; targets multiples of 1/4
  const int n = 61, d = 5;
  uint64_t s = 0x5A17E001;
  std::vector<int> A((size_t)n * d);
  for (int& a : A) a = (int)(splitmix64(s) % 7) - 3;
  std::vector<double> K((size_t)n * n), y(n), target(n);
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) {
      long v = 0;
      for (int k = 0; k < d; ++k) v += (long)A[r * d + k] * A[c * d + k];
      K[(size_t)r * n + c] = std::ldexp((double)v, -2);
    }
  for (int r = 0; r < n; ++r) {
    y[r] = (r % 3 == 0) ? 1.0 : -1.0;
    target[r] = ((int)(splitmix64(s) % 65) - 32) / 4.0;
  }
  // a permuted partial training list that ends at the Gram's last example
  std::vector<int32_t> train, test;
  for (int k = 0; k < 47; ++k) train.push_back((k * 37 + 60) % n);
  for (int k = 0; k < n; k += 4) test.push_back(n - 1 - k);

  int failures = 0;
  std::vector<sk_svm_task> tasks;
  for (int type = SK_SVM_C_SVC; type <= SK_SVM_NU_SVR; ++type) {
    sk_svm_task T = {train.data(), (int32_t)train.size(), test.data(), (int32_t)test.size(), type, 0.5, 0.3, 0.25,
                     1e-3, 100000};
    tasks.push_back(T);
  }
  // one task per call, exact-size outputs; SVR on targets, the classifiers on labels
  std::vector<std::vector<double>> coefs;
  for (const sk_svm_task& T : tasks) {
    const bool svr = T.svm_type == SK_SVM_EPSILON_SVR || T.svm_type == SK_SVM_NU_SVR;
    std::vector<double> coef(train.size()), dec(test.size());
    sk_svm_task_solution S;
    const int rc = sk_svm_solve_batch_host(K.data(), n, T.svm_type == SK_SVM_ONE_CLASS ? nullptr
                                                         : svr                         ? target.data()
                                                                                       : y.data(),
                                           &T, 1, 1, coef.data(), dec.data(), &S);
    int nsv = 0;
    for (double c : coef) nsv += c != 0.0;
    std::printf("type %d: rc %d status %d iterations %lld nSV %d rho %.6g obj %.6g r %.6g\n", T.svm_type, rc,
                S.status, (long long)S.iterations, nsv, S.rho, S.obj, S.r);
    if (rc != SK_OK || S.status != SK_SVM_CONVERGED || nsv < 2 || !std::isfinite(S.rho) || !std::isfinite(dec[0]))
      ++failures;
    coefs.push_back(coef);
  }
  // all five in one call on three threads, on one target array whose signs are
  // the labels; the classifiers and one-class must give the same coefficients
  std::vector<double> both(n);
  for (int r = 0; r < n; ++r) both[r] = y[r] * (std::fabs(target[r]) + 1.0);
  std::vector<double> coef(tasks.size() * train.size()), dec(tasks.size() * test.size());
  std::vector<sk_svm_task_solution> sol(tasks.size());
  const int rc = sk_svm_solve_batch_host(K.data(), n, both.data(), tasks.data(), (int32_t)tasks.size(), 3, coef.data(),
                                         dec.data(), sol.data());
  if (rc != SK_OK) ++failures;
  for (int type = SK_SVM_C_SVC; type <= SK_SVM_ONE_CLASS; ++type)
    for (size_t k = 0; k < train.size(); ++k)
      if (coef[type * train.size() + k] != coefs[type][k]) {
        ++failures;
        break;
      }
  // refusals return before anything is written
  sk_svm_task bad = tasks[SK_SVM_NU_SVR];
  bad.nu = 1.5;
  if (sk_svm_solve_batch_host(K.data(), n, target.data(), &bad, 1, 1, coef.data(), dec.data(), sol.data()) !=
      SK_ERR_INVALID)
    ++failures;
  failures += c_svc_with_and_without_shrinking();
  if (failures) {
    std::printf("FAILED: %d\n", failures);
    return 1;
  }
  std::printf("ok: 5 types\n");
  return 0;
}
