// Device pieces of the McCaskill loop model shared by the fold kernel
// (fold.hip) and the structure sampler (fold_sample.hip): the sampler's
// candidates are the terms of the fold's inside sums, so both must read the
// same pair types and loop factors.  The block / team sums and the ring size
// are shared with the consensus fold (fold_ali.hip), whose passes are the
// fold's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fold_ali_model.h"  // kFoldPairBits: the pair-type table

namespace sk {

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

// block-wide sum (at most 8 waves), result in every thread
__device__ __forceinline__ double block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int k = 0; k < nw; ++k) s += red[k];
  return s;
}

// sum over a team of G (1, 2, 4, 8) adjacent lanes, in every lane of the team
__device__ __forceinline__ double team_sum(double v, int G) {
  if (G >= 2) v += __shfl_xor(v, 1, 64);
  if (G >= 4) v += __shfl_xor(v, 2, 64);
  if (G >= 8) v += __shfl_xor(v, 4, 64);
  return v;
}

// lanes per cell of a span of ncell cells: the most (up to 8) that keep
// every cell of the span in one pass of the block's threads
__device__ __forceinline__ int team_of(int ncell, int nt) {
  int G = 1;
  while (G < 8 && ncell * (2 * G) <= nt) G *= 2;
  return G;
}

// LDS ring of the interior-loop window (fold.hip, fold_ali.hip)
constexpr int kFoldRing = 33;  // 31 diagonals read + the one written, distinct slots

}  // namespace sk
