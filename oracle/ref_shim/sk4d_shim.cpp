// Harness for oracle/_ref/libskref_4d.so: the reference's own, unmodified
// stem_kernel/stem_kernel.cpp and stem_kernel/phmm.cpp, compiled in place by
// oracle/Makefile against the stand-in headers, behind a C ABI.
//
// StemKernel<ValueType, BPMat> is a template whose member definitions live in
// stem_kernel.cpp, so that file is included here (from the reference tree, by
// the include path) and instantiated with a BPMat of this file that serves
// base-pairing probabilities injected by the caller -- the place the
// reference's own BPMatrix (PFWrapper / ViennaRNA, HAVE_LIBRNA) would take.
// full_dp, partial_dp, alignment_constraints and the PairHMM are the
// reference's code.
#include <algorithm>
#include <cassert>
#include <cstring>
#include <deque>
#include <iostream>
#include <list>
#include <string>
#include <utility>
#include <vector>
// alignment_constraints is a private member; the test compares its output.
#define private public
#include "stem_kernel.h"
#undef private
#include "stem_kernel.cpp"

namespace {
struct Injected {
  const std::string* seq;
  const double* packed;  // strict upper triangle, row-major; 0 = no pairs
};
Injected g_inj[2] = {{0, 0}, {0, 0}};
}  // namespace

// Stands for the reference's HAVE_LIBRNA BPMatrix (stem_kernel.cpp): prob()
// there is PFWrapper's pr(i+1, j+1) returned as float, 0 on the diagonal.
class InjectedBPMat {
 public:
  InjectedBPMat(const std::string& seq, uint, bool) : n_(seq.size()), p_(0) {
    for (int k = 0; k != 2; ++k)
      if (g_inj[k].seq == &seq) p_ = g_inj[k].packed;
  }
  float prob(uint i, uint j) {
    if (!p_ || i >= j) return 0.0f;
    return p_[(size_t)i * n_ - (size_t)i * (i + 1) / 2 + (j - i - 1)];
  }

 private:
  size_t n_;
  const double* p_;
};

template class StemKernel<double, InjectedBPMat>;

extern "C" {

// StemKernel::operator(): full_dp, or partial_dp when band or ali_bound is
// set.  model 0: injected probabilities; 1: NormalBasePair; 2: WobbleBasePair.
double sk4_kernel(const char* xs, const double* bpx, const char* ys, const double* bpy, double gap,
                  double stack, double subst, float bp_bound, int model, unsigned loop,
                  unsigned band, float ali_bound) {
  const std::string x(xs), y(ys);
  if (model == 1)
    return StemKernel<double, NormalBasePair>(false, loop, gap, stack, subst, band, ali_bound,
                                              bp_bound)(x, y);
  if (model == 2)
    return StemKernel<double, WobbleBasePair>(true, loop, gap, stack, subst, band, ali_bound,
                                              bp_bound)(x, y);
  g_inj[0].seq = &x;
  g_inj[0].packed = bpx;
  g_inj[1].seq = &y;
  g_inj[1].packed = bpy;
  const double v = StemKernel<double, InjectedBPMat>(false, loop, gap, stack, subst, band,
                                                     ali_bound, bp_bound)(x, y);
  g_inj[0] = g_inj[1] = Injected();
  return v;
}

// PairHMM<>::forward_backward: fb[s][i][j], s = M, IX, IY.
void sk4_phmm_posterior(const char* xs, const char* ys, double* fb) {
  const std::string x(xs), y(ys);
  PairHMM<> phmm;
  PairHMM<>::FBTable tb;
  phmm.forward_backward(x, y, tb);
  const size_t n = x.size() + 1, m = y.size() + 1;
  for (size_t s = 0; s != 3; ++s)
    for (size_t i = 0; i != n; ++i)
      for (size_t j = 0; j != m; ++j) fb[(s * n + i) * m + j] = tb[s][i][j];
}

// StemKernel::alignment_constraints: c_low / c_high, |x|+1 each.
void sk4_alignment_constraints(const char* xs, const char* ys, float ali_bound, unsigned band,
                               unsigned* c_low, unsigned* c_high) {
  const std::string x(xs), y(ys);
  StemKernel<double, NormalBasePair> k(false, 3, 0.8, 1.0, 0.5, band, ali_bound, 0.0f);
  std::vector<uint> lo, hi;
  k.alignment_constraints(x, y, lo, hi);
  std::copy(lo.begin(), lo.end(), c_low);
  std::copy(hi.begin(), hi.end(), c_high);
}
}
