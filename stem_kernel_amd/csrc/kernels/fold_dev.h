// Device pieces the fold kernels share.  fold.hip and fold_ali.hip run the
// same passes over tables of one layout (FoldWork, launch.h): the passes are
// here once, and where the two differ by a factor a per-kernel pair model
// supplies it (FoldPairModel; fold_ali.hip's answers 1).  The interior-loop
// sums differ in substance and stay in the kernels.  The sampler
// (fold_sample.hip) walks the terms of the fold's inside sums, so it reads
// the same pair types and loop factors.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fold_ali_model.h"  // kFoldPairBits: the pair-type table
#include "launch.h"

namespace sk {

struct FoldTables {  // views into P.tab (FoldLaunch::tab layout)
  const double *st, *hp, *bu, *in, *ni, *au, *scp;
  double mlc, mli;
};

// the views of a launch's tables: tl the LDS copy, big where the two tables
// sized by the longest sequence (hairpin, scale powers) are read from (tl, or
// P.tab for a launch that leaves them in HBM)
__device__ __forceinline__ FoldTables fold_table_views(const FoldLaunch& P, const double* tl, const double* big) {
  FoldTables T;
  T.st = tl + P.o_st;
  T.hp = big + P.o_hp;
  T.bu = tl + P.o_bu;
  T.in = tl + P.o_in;
  T.ni = tl + P.o_ni;
  T.au = tl + P.o_au;
  T.scp = big + P.o_scp;
  T.mlc = tl[P.o_ml];
  T.mli = tl[P.o_ml + 1];
  return T;
}

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

// The pair model of the single-sequence fold (codes c, the --noLonelyPairs
// host table lp or nullptr, --noGU, --noClosingGU), and what the shared passes
// ask of a kernel about a pair: branch, the terminal factor of (i, l) as a
// multiloop or exterior branch; closer, that of (i, j) closing a multiloop,
// or 0 where it may not.
struct FoldPairModel {
  const int8_t* c;
  const uint8_t* lp;
  const double* au;
  int n;
  bool ngu, ncg;
  __device__ __forceinline__ int ptype(int i, int j) const { return fold_ptype(c, lp, n, ngu, i, j); }
  __device__ __forceinline__ double branch(int i, int l) const { return au[pair_raw(c[i], c[l])]; }
  __device__ __forceinline__ double closer(int i, int j) const {
    const int t = ptype(i, j);
    return (!t || (ncg && is_gu(t))) ? 0.0 : au[t];
  }
};

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

// LDS ring of the interior-loop window (fold.hip, fold_ali.hip): the slot of
// diagonal d, and the slot of d - 1 / d + 1 given d's
constexpr int kFoldRing = 33;  // 31 diagonals read + the one written, distinct slots
__device__ __forceinline__ int fold_ring_slot(int d) { return d % kFoldRing; }
__device__ __forceinline__ int fold_ring_dn(int sl) { return sl == 0 ? kFoldRing - 1 : sl - 1; }
__device__ __forceinline__ int fold_ring_up(int sl) { return sl == kFoldRing - 1 ? 0 : sl + 1; }

// The passes below run per cell (i, j) of a span on lane r of the cell's team
// of G; on: the cell exists (threads past the span's last cell idle on cell 0
// and store nothing).
// Inside, after Qb(i, j) (qb: the cell's own, which the other lanes of the
// team do not see in memory yet):
//   Qm1(i, j): Qb(i, l) closing the branch, l = i+4 .. j
//   Qm(i, j) = sum_u (sc^(u-i) + Qm(i, u-1)) Qm1(u, j)
template <class Model>
__device__ __forceinline__ void fold_qm_updates(const FoldWork& w, const FoldTables& T, const Model& M,
                                                int i, int j, int r, int G, bool on, double qb) {
  double m1 = 0.0, m = 0.0;
  if (on) {
#pragma unroll 4
    for (int l = i + 4 + r; l <= j; l += G) {
      const double v = l == j ? qb : w.qb(l - i, i);
      if (v != 0.0) m1 += v * T.mli * M.branch(i, l) * T.scp[j - l];
    }
  }
  m1 = team_sum(m1, G);
  if (on && r == 0) w.qm1(j - i, i) = m1;
  if (on) {
#pragma unroll 4
    for (int u = i + r; u + 4 <= j; u += G)
      m += (T.scp[u - i] + (u - 1 >= i ? w.qm(u - 1 - i, i) : 0.0)) * (u == i ? m1 : w.qm1(j - u, u));
  }
  m = team_sum(m, G);
  if (on && r == 0) w.qm(j - i, i) = m;
}

// Exterior: Q5[j+1] = Q5[j] sc + sum_k Q5[k] Qb(k, j) (branch); returns Z = Q5[n]
template <class Model>
__device__ __forceinline__ double fold_q5_sweep(const FoldWork& w, const FoldTables& T, const Model& M, double* red) {
  const int n = (int)w.n, tid = threadIdx.x, nt = blockDim.x;
  double* Q5 = w.q5();
  if (tid == 0) Q5[0] = 1.0;
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    double s = 0.0;
    for (int k = tid; k + 4 <= j; k += nt) {
      const double v = w.qb(j - k, k);
      if (v != 0.0) s += Q5[k] * v * M.branch(k, j);
    }
    s = block_sum(s, red);
    if (tid == 0) Q5[j + 1] = Q5[j] * T.scp[1] + s;
    __syncthreads();
  }
  return Q5[n];
}

// its adjoint: H5[k] = H5[k+1] sc + sum_j H5[j+1] Qb(k, j) (branch)
template <class Model>
__device__ __forceinline__ void fold_h5_sweep(const FoldWork& w, const FoldTables& T, const Model& M, double* red) {
  const int n = (int)w.n, tid = threadIdx.x, nt = blockDim.x;
  double* H5 = w.h5();
  if (tid == 0) H5[n] = 1.0;
  __syncthreads();
  for (int k = n - 1; k >= 0; --k) {
    double s = 0.0;
    for (int j = k + 4 + tid; j < n; j += nt) {
      const double v = w.qb(j - k, k);
      if (v != 0.0) s += H5[j + 1] * v * M.branch(k, j);
    }
    s = block_sum(s, red);
    if (tid == 0) H5[k] = H5[k + 1] * T.scp[1] + s;
    __syncthreads();
  }
}

// Outside, before Hb(i, j); returns Hm1(i, j):
//   Hm(i,j):  Qm(i,j2) += Qm(i,j) Qm1(j+1,j2);  Qb(i-1,j') ML rule with u = j
//   Hm1(i,j): Qm(ii,j) += (sc^(i-ii) + Qm(ii,i-1)) Qm1(i,j), ii <= i;
//             Qb(i',j+1) ML rule with u + 1 = i
//   (ii = i - e, e up: the threads read consecutive doubles)
template <class Model>
__device__ __forceinline__ double fold_hm_updates(const FoldWork& w, const FoldTables& T, const Model& M,
                                                  int i, int j, int r, int G, bool on) {
  const int n = (int)w.n, d = j - i;
  double hm = 0.0, hm1 = 0.0;
  if (on) {
#pragma unroll 4
    for (int j2 = j + 5 + r; j2 < n; j2 += G) hm += w.hm(j2 - i, i) * w.qm1(j2 - j - 1, j + 1);
    if (i >= 1) {
      for (int jp = j + 6 + r; jp < n; jp += G) {
        const double v = w.hb(jp - i + 1, i - 1);
        const double a = v != 0.0 ? M.closer(i - 1, jp) : 0.0;
        if (a != 0.0) hm += v * T.mlc * a * T.scp[2] * w.qm1(jp - j - 2, j + 1);
      }
    }
  }
  hm = team_sum(hm, G);
  if (on && r == 0) w.hm(d, i) = hm;
  if (on) {
#pragma unroll 4
    for (int e = r; e <= i; e += G) {
      const double v = e == 0 ? hm : w.hm(d + e, i - e);
      if (v != 0.0) hm1 += v * (T.scp[e] + (e >= 1 ? w.qm(e - 1, i - e) : 0.0));
    }
    if (j + 1 < n) {
      for (int e = 6 + r; e <= i; e += G) {  // ip = i - e
        const double v = w.hb(d + 1 + e, i - e);
        const double a = v != 0.0 ? M.closer(i - e, j + 1) : 0.0;
        if (a != 0.0) hm1 += v * T.mlc * a * T.scp[2] * w.qm(e - 2, i - e + 1);
      }
    }
  }
  hm1 = team_sum(hm1, G);
  if (on && r == 0) w.hm1(d, i) = hm1;
  return hm1;
}

// One launch wrapper for the three kernels
template <class Launch>
static hipError_t launch_fold_kernel(void (*kernel)(Launch), const Launch& P, dim3 grid, int threads, size_t lds,
                                     hipStream_t st) {
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, st, P);
  return hipGetLastError();
}

}  // namespace sk
