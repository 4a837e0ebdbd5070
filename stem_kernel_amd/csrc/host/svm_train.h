// C-SVC training: what the host path (svm_train.cpp) and the GPU path
// (kernels/svm_smo.hip) share.  Not part of the ABI.
#pragma once

#include <cstdint>
#include <string>

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

}  // namespace sk
