// Device pieces of the McCaskill loop model shared by the fold kernel
// (fold.hip) and the structure sampler (fold_sample.hip): the sampler's
// candidates are the terms of the fold's inside sums, so both must read the
// same pair types and loop factors.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sk {

// pair type of codes (a, b), a * 4 + b -> 4 bits of a 64-bit constant (no
// memory access: a __constant__ table indexed per thread is a vector load):
// {0,0,0,5, 0,0,1,0, 0,2,0,4, 6,0,3,0}  CG1 GC2 GU3 UG4 AU5 UA6
constexpr uint64_t kFoldPairBits = 0x306402001005000ull;

struct FoldTables {  // views into P.tab (FoldLaunch::tab layout)
  const double *st, *hp, *bu, *in, *ni, *au, *scp;
  double mlc, mli;
};

__device__ __forceinline__ int pair_raw(int a, int b) {
  return (a < 0 || b < 0) ? 0 : (int)((kFoldPairBits >> (4 * (a * 4 + b))) & 0xfu);
}
__device__ __forceinline__ bool is_gu(int t) { return t == 3 || t == 4; }

// pair type of (i, j) under --noLonelyPairs (host table lp, nullptr: off) and --noGU
__device__ __forceinline__ int fold_ptype(const int8_t* c, const uint8_t* lp, int n, bool ngu, int i, int j) {
  const int t = pair_raw(c[i], c[j]);
  if (lp && !lp[(size_t)i * n + j]) return 0;
  return (ngu && is_gu(t)) ? 0 : t;
}

// interior / bulge / stack loop factor (unscaled), t1 = type(i,j), t2 = type(q,p)
__device__ __forceinline__ double fold_interior(const FoldTables& T, int t1, int t2, int n1, int n2,
                                                bool ncg) {
  const int n = n1 + n2;
  if (n == 0) return T.st[t1 * 7 + t2];
  if (ncg && (is_gu(t1) || is_gu(t2))) return 0.0;
  if (n1 == 0 || n2 == 0) return n == 1 ? T.bu[1] * T.st[t1 * 7 + t2] : T.bu[n] * T.au[t1] * T.au[t2];
  return T.in[n] * T.ni[abs(n1 - n2)] * T.au[t1] * T.au[t2];
}

}  // namespace sk
