// SVM training (C-SVC, and the four other formulations of svm_train_one): what
// the host path (svm_train.cpp) and the GPU path (kernels/svm_smo.hip) share.
// Not part of the ABI.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/stem_kernel.h"

namespace sk {

// size classes of the GPU solver: threads of the workgroup; every thread owns
// kSvmElems training examples (k = tid, tid + T, ...)
constexpr int kSvmClasses = 3;
constexpr int kSvmElems = 4;
constexpr int kSvmThreads[kSvmClasses] = {64, 256, 1024};
constexpr int kSvmMaxTrain = kSvmThreads[kSvmClasses - 1] * kSvmElems;

// The longest training list of a type on the GPU: the SVR types have 2 l positions.
constexpr int svm_type_max_train(int svm_type) {
  return svm_type == SK_SVM_EPSILON_SVR || svm_type == SK_SVM_NU_SVR ? kSvmMaxTrain / 2 : kSvmMaxTrain;
}
constexpr bool svm_type_is_svr(int t) { return t == SK_SVM_EPSILON_SVR || t == SK_SVM_NU_SVR; }
constexpr bool svm_type_is_nu(int t) { return t == SK_SVM_NU_SVC || t == SK_SVM_NU_SVR; }

// One problem as the checks, the host solver and the GPU's batch builder see
// it: an sk_svm_problem (C-SVC with Cp and Cn) or an sk_svm_task (Cp = Cn = C).
struct SvmJob {
  const int32_t* train;
  int32_t n_train;
  const int32_t* test;
  int32_t n_test;
  int32_t svm_type;
  double Cp, Cn, nu, p, eps;
  int64_t max_iter;
};
inline SvmJob svm_job(const sk_svm_problem& P) {
  return {P.train, P.n_train, P.test, P.n_test, SK_SVM_C_SVC, P.Cp, P.Cn, 0.0, 0.0, P.eps, P.max_iter};
}
inline SvmJob svm_job(const sk_svm_task& T) {
  return {T.train, T.n_train, T.test, T.n_test, T.svm_type, T.C, T.C, T.nu, T.p, T.eps, T.max_iter};
}
// The jobs of a call's array; none for a null array, which svm_check_jobs refuses.
template <class T>
std::vector<SvmJob> svm_jobs(const T* items, int32_t count) {
  std::vector<SvmJob> jobs;
  for (int32_t p = 0; items && p < count; ++p) jobs.push_back(svm_job(items[p]));
  return jobs;
}

// The two calls as the checks name them in their messages; typed: the jobs
// carry an svm_type of the caller's (sk_svm_task).
struct SvmCall {
  const char* name;
  const char* noun;
  bool typed;
};
constexpr SvmCall kSvmTrainBatch = {"sk_svm_train_batch", "problem", false};
constexpr SvmCall kSvmSolveBatch = {"sk_svm_solve_batch", "task", true};

// The argument checks of sk_svm_train_batch[_host][_ex] and
// sk_svm_solve_batch[_host]: SK_OK, or SK_ERR_INVALID with the reason in err.
// n_jobs is the caller's count, out its alpha_out or coef_out.  on_gpu: a
// training list over its type's limit is SK_ERR_UNSUPPORTED.  *sum_train /
// *sum_test: lengths of the outputs.
int svm_check_jobs(const SvmCall& call, const double* gram, int32_t n, const double* targets,
                   const std::vector<SvmJob>& jobs, int32_t n_jobs, const double* out, const double* dec_out,
                   const void* solutions, bool on_gpu, int64_t* sum_train, int64_t* sum_test, std::string& err);

// A job as the solver sees it, built as the reference's solve_* builds it
// (svm.cpp:38-234): per position the Gram index and y packed as
// (index << 1) | (y > 0), the linear term and the starting alpha; *Cp / *Cn:
// the upper bound of the positions with y = +1 / y = -1 (one C for both but
// for C-SVC).  Appends to the vectors and returns the number of positions (l,
// or 2 l for SVR).
int svm_task_positions(const double* targets, const SvmJob& J, std::vector<int32_t>& ty, std::vector<double>& p,
                       std::vector<double>& alpha0, double* Cp, double* Cn);

}  // namespace sk
