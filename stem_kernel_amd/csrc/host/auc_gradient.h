// Cross-validated AUC gradient: what the host path (auc_gradient.cpp) and the
// GPU path (kernels/auc_grad.hip) share.  Not part of the ABI.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/stem_kernel.h"

namespace sk {

// The GPU path's two classes, by N = n_free + 1 (the side of the KKT system):
// N <= kAucLdsN keeps P in LDS beside the vectors (256 threads); a larger
// system keeps P in a device scratch and only the four CG vectors in LDS
// (1,024 threads).  LDS of a workgroup: kAucStage staging doubles, 4 N
// vector doubles and, in the first class, N^2 doubles of P:
//   8 (1,024 + 4*136 + 136^2) = 160,512 B of the CU's 163,840, and
//   8 (1,024 + 4*4,096)       = 139,264 B in the second class.
constexpr int kAucLdsN = 136;
constexpr int kAucMaxN = 4096;
constexpr int kAucStage = 1024;
constexpr int kAucThreadsLds = 256, kAucThreadsScratch = 1024;
// P scratch: 8 N^2 bytes per problem (128 MiB at kAucMaxN, the most one
// problem may take); the problems of one launch share kAucScratchBudget.
constexpr int64_t kAucScratchPerProblem = (int64_t)8 * kAucMaxN * kAucMaxN;
constexpr int64_t kAucScratchBudget = (int64_t)1 << 30;

// The argument checks of sk_auc_gradient_batch[_host]: SK_OK, or
// SK_ERR_INVALID with the reason in err.  n_free[p] / n_bound[p] are counted
// as find_support_vectors does; max_n > 0: a problem with n_free + 1 > max_n
// is SK_ERR_UNSUPPORTED.
int auc_check_batch(const double* gram, const double* grads, int32_t n_params, int32_t n, const double* labels,
                    const sk_auc_problem* problems, int32_t n_problems, const double* cg_out,
                    const double* fg_out, const sk_auc_info* info, int32_t max_n, std::vector<int32_t>& n_free,
                    std::vector<int32_t>& n_bound, std::string& err);

// finite = 1 when cg, every fg and every written d_u entry is finite
int32_t auc_outputs_finite(double cg, const double* fg, int32_t n_params, const double* d_u, int32_t n_du);

}  // namespace sk
