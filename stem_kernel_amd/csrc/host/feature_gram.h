// Feature-vector Grams (the reference's rbf/poly/sigmoid optimizers,
// optimizer/{rbf,poly,sigmoid}_kernel.cpp): the feature set behind the
// sk_features handle, the shape constants, and the one epilogue both paths
// compile -- csrc/host/feature_gram.cpp with libm, csrc/kernels/feature_gram.hip
// with the device's exp/tanh/cosh.  Not part of the ABI.
//
// Exactness of the dot matrix.  The reference's dot() is libsvm's sparse merge:
// sum = 0, then sum += x.value * y.value for every index both vectors hold, in
// ascending index order, the multiply and the add rounded separately.  Here an
// example is dense over the compacted columns (the sorted union of the indices
// in use, mapped order-preservingly to 0..d-1; absent entries +0) and the dot
// is the in-order sum of x_k * y_k over all d columns from +0.  With finite
// values the two are the same bits: a column absent from either vector
// contributes x_k * y_k = +-0, and adding +-0 never changes the running sum --
// a nonzero sum is unchanged, and the sum is never -0 (it starts at +0; +0 + -0
// is +0 in round-to-nearest; an exact cancellation gives +0; an addition never
// underflows to zero), so +0 + +-0 stays +0.  The columns the vectors share are
// visited in the same ascending order.  That is why non-finite values are
// refused (0 * inf is NaN) and why both files are compiled with
// -ffp-contract=off (an FMA would round the multiply and the add together).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define SK_FEAT_HD __host__ __device__
#else
#define SK_FEAT_HD
#endif

struct sk_context;

// Immutable once created (the resident dot matrices rely on it).
struct sk_features {
  int32_t n = 0;
  std::vector<int64_t> row_ptr;  // n + 1
  std::vector<int32_t> index;    // as given: ascending within a row, >= 0
  std::vector<double> value;     // finite
  std::vector<int32_t> labels;   // n
  std::vector<int32_t> cols;     // the sorted union of the indices in use (d entries)
};

namespace sk {

// feat_dot: one workgroup of kFeatThreads computes a kFeatTile x kFeatTile tile
// of outputs, each thread a kFeatReg x kFeatReg block in registers; the X and Y
// panels of a k-slice of kFeatSlice columns are double-buffered in LDS.
constexpr int kFeatTile = 64, kFeatSlice = 16, kFeatReg = 4, kFeatThreads = 256;
// Limits, from the memory a call needs.  n: the resident D, K and two gradient
// matrices are 4 n^2 doubles on the device and (1 + P) n^2 on the host: 8 GiB
// at 16,384.  Dense budget: the examples of a call (both sets of a cross call)
// over their compacted columns, n d doubles on the host and on the device:
// 2 GiB at 2^28.
constexpr int32_t kFeatMaxN = 16384;
constexpr int64_t kFeatMaxDense = (int64_t)1 << 28;
// dot matrices a context keeps resident (the oldest is dropped)
constexpr int kFeatResident = 4;

enum { kFeatRbf = 0, kFeatPoly = 1, kFeatSigmoid = 2 };
inline int feat_n_params(int kind) { return kind == kFeatRbf ? 1 : 2; }

// libsvm's powi (poly_kernel.cpp:13-24): square and multiply, plain multiplies
SK_FEAT_HD inline double feat_powi(double base, int times) {
  double tmp = base, ret = 1.0;
  for (int t = times; t > 0; t /= 2) {
    if (t % 2 == 1) ret *= tmp;
    tmp = tmp * tmp;
  }
  return ret;
}

// One entry's K and gradients from d = dot(x, y), dii = dot(x, x), djj =
// dot(y, y), operation for operation what the reference's kernel() and
// kernel_g() do.  g1 is not written for the RBF kernel.
template <int KIND>
SK_FEAT_HD inline void feat_entry(double d, double dii, double djj, int degree, double p0, double p1, double& k,
                                  double& g0, double& g1) {
  if (KIND == kFeatRbf) {
    const double w = (dii + djj) - 2 * d;  // dot(x,x)+dot(y,y)-2*dot(x,y)
    const double e = exp(-p0 * w);
    k = e;
    g0 = -w * e;
  } else if (KIND == kFeatPoly) {
    const double t = p0 * d + p1;
    k = feat_powi(t, degree);
    const double v = feat_powi(t, degree - 1) * degree;
    g0 = v * d;
    g1 = v;
  } else {
    const double t = p0 * d + p1;
    k = tanh(t);
    const double w = cosh(t);
    const double v = 1.0 / (w * w);
    g0 = v * d;
    g1 = v;
  }
}

// the union of two sets' columns (ys may be null: xs's own), and a set's
// examples dense over it, row-major n x cols.size(), absent entries +0
std::vector<int32_t> feat_columns(const sk_features* xs, const sk_features* ys);
void feat_dense(const sk_features* fs, const std::vector<int32_t>& cols, double* out);
// argument and limit checks shared by the host and GPU entry points: 0, or a
// status with the message in err.  ys null: the symmetric case.
int feat_check(const char* who, const sk_features* xs, const sk_features* ys, int kind, int degree,
               const double* params, bool need_params, std::string& err);
void feat_set_error(const std::string& msg);
// resident dot matrices (csrc/kernels/feature_gram.hip): dropped when their
// context closes or one of their sets is freed
void feat_dots_forget(const sk_context* ctx, const sk_features* fs);

}  // namespace sk
