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

// The argument checks of sk_svm_train_batch[_host]: SK_OK, or SK_ERR_INVALID
// with the reason in err.  max_train > 0: a longer training list is
// SK_ERR_UNSUPPORTED.  *sum_train / *sum_test: lengths of the outputs.
int svm_check_batch(const double* gram, int32_t n, const double* labels, const sk_svm_problem* problems,
                    int32_t n_problems, const double* alpha_out, const double* dec_out,
                    const sk_svm_solution* solutions, int32_t max_train, int64_t* sum_train,
                    int64_t* sum_test, std::string& err);

// ---- the five formulations (sk_svm_solve_batch[_host])

// The longest training list of a type on the GPU: the SVR types have 2 l positions.
constexpr int svm_type_max_train(int svm_type) {
  return svm_type == SK_SVM_EPSILON_SVR || svm_type == SK_SVM_NU_SVR ? kSvmMaxTrain / 2 : kSvmMaxTrain;
}
constexpr bool svm_type_is_svr(int t) { return t == SK_SVM_EPSILON_SVR || t == SK_SVM_NU_SVR; }
constexpr bool svm_type_is_nu(int t) { return t == SK_SVM_NU_SVC || t == SK_SVM_NU_SVR; }

// The argument checks of sk_svm_solve_batch[_host]; on_gpu: a list over its
// type's limit is SK_ERR_UNSUPPORTED.
int svm_check_tasks(const double* gram, int32_t n, const double* targets, const sk_svm_task* tasks, int32_t n_tasks,
                    const double* coef_out, const double* dec_out, const sk_svm_task_solution* solutions,
                    bool on_gpu, int64_t* sum_train, int64_t* sum_test, std::string& err);

// A task of one of the four new types as the solver sees it, built as the
// reference's solve_* builds it (svm.cpp:73-234): per position the Gram index
// and y packed as (index << 1) | (y > 0), the linear term and the starting
// alpha; one bound C for all positions.  Appends to the vectors and returns
// the number of positions (l, or 2 l for SVR).
int svm_task_positions(const double* targets, const sk_svm_task& T, std::vector<int32_t>& ty,
                       std::vector<double>& p, std::vector<double>& alpha0, double* C);

}  // namespace sk
