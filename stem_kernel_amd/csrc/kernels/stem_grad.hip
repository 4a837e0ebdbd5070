// Gradients of the DAG stem kernels with respect to their own parameters
// (gfx950): value and d/d(loop_gap, beta) of the Su kinds (NP = 2), value and
// d/d(loop_gap, stack, covar) of the Si kinds (NP = 3).
//
// Reference: StemKernel<ST,MData>::operator()  stem_kernel_lite/stem_kernel.cpp:14-95
// (node scores score_table.cpp:14-53, 118-201; edge scores :60-101),
// differentiated in forward mode: the reference has no gradient of this DP.
//
// The schedule is sk_dag_stem_big_kernel's (dag_stem_big.hip: K never stored,
// K = P_x M P_y; leaf rows / columns in closed form; one weighted child row S
// per x row; the y DAG read in level order from the packed x-role arrays),
// with every per-row vector carried as 1 + NP vectors, component 0 the value
// and component 1 + p the tangent of parameter p (p = 0: loop_gap):
//   A. S[q]  = sum_{c in ch(p)} g^gaps G0[c][q]
//   B. level by level (children first), a pull per node, no atomics:
//        M[q]  = node_score(p,q) * H[q] inside the length band,
//        H[q]  = sum_{cy in ch(q)} g^gy S[cy]   (loop q: closed form),
//        G1[q] = M[q] + sum_{cy} G1[cy] * (gap^2 w_y(q)) * g^gy,
//        K    += P_x[p] * M[q] * P_y[q];
//   C. G0[p][q] = G1[q] + v_s(p) S[q] -> p's recycled slot.
// The inputs' tangents: d g^k = k g^(k-1) and d gap^2 = 2 gap (host tables),
// d co_subst = ribosum * co_subst (Su, host table), the code-equality
// indicators (Si), and the leaf closed forms' (sk_stem_grad_prep_kernel).
// One wavefront per pair; the lanes of a wave exchange S / G1 through global
// memory, so the phases are separated by workgroup-scope fences.  Component c
// of row vector V is V[c * stride + q]: a slab row is (1 + NP) * stride
// doubles.
#include <hip/hip_runtime.h>

#include "device_set.h"
#include "launch.h"

namespace sk {
namespace {

__device__ __forceinline__ void grad_lane_exchange_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Per call: L[p] = G0[p][y-leaf column], SL[p] = sum_e g^gaps L[child] and
// their d/dloop_gap (one thread per example, nodes in level order = children
// first), as sk_prep_kernel (dag_stem.hip) forms the values.
__global__ void sk_stem_grad_prep_kernel(StemGradPrep P) {
  const DevSet& s = P.s;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= s.n_examples) return;
  const int nl = s.ex_nl[e];
  const int nb = s.ex_node_base[e], eb = s.ex_edge_base[e];
  for (int k = 0; k < nl; ++k) {
    const uint32_t a = s.nd_a[nb + k];
    const int e0 = a & 0xffff, ne = (a >> 16) & 0xff;
    const double w = (double)s.nd_w[nb + k];
    const double v_s = P.gap2 * w, dv_s = P.dgap2 * w;
    double L = 0.0, dL = 0.0, SL = 0.0, dSL = 0.0;
    if (ne == 0) {  // loop node: its single child is a leaf (G0[leaf][leaf] = 1)
      const uint32_t g = s.nd_c[nb + k];
      L += 1.0 * v_s * P.gpow[g];
      dL += dv_s * P.gpow[g] + v_s * P.dgpow[g];
    } else {
      for (int t = 0; t < ne; ++t) {
        const uint32_t ed = s.ed[eb + e0 + t].x;
        const double gp = P.gpow[ed >> 16], dgp = P.dgpow[ed >> 16];
        const double Lc = P.nd_L[nb + (ed & 0xffff)], dLc = P.nd_dL[nb + (ed & 0xffff)];
        L += Lc * v_s * gp;
        dL += (dLc * v_s + Lc * dv_s) * gp + Lc * v_s * dgp;
        SL += gp * Lc;
        dSL += dgp * Lc + gp * dLc;
      }
    }
    P.nd_L[nb + k] = L;
    P.nd_dL[nb + k] = dL;
    P.nd_SL[nb + k] = SL;
    P.nd_dSL[nb + k] = dSL;
  }
  for (int r = 0; r < nl; ++r) {
    const uint32_t k = s.xr_node[nb + r];
    P.xr_SL[nb + r] = P.nd_SL[nb + k];
    P.xr_dSL[nb + r] = P.nd_dSL[nb + k];
  }
}

// node_match_score (score_table.cpp:162-201 Subst / :14-53 Simple) and its
// tangents: v[0] the score, v[1] d/dloop_gap (the two gap-column terms),
// v[2] d/dbeta (NP = 2) or v[2], v[3] d/dstack, d/dcovar (NP = 3).
template <int NP>
__device__ __forceinline__ void grad_node_score(double* v, const double* __restrict__ co,
                                                const double* __restrict__ dco, const DevSet& xs, int xbf,
                                                int xnbf, double x_nbp, double x_nseq, double xw,
                                                const DevSet& ys, int ybf, int ynbf, double y_nbp,
                                                double y_nseq, double yw, double gap2, double dgap2) {
#pragma unroll
  for (int c = 0; c <= NP; ++c) v[c] = 0.0;
  for (int a = 0; a < xnbf; ++a) {
    const double cx = (double)xs.bpf_p[xbf + a];
    const uint32_t xc = xs.bpf_code[xbf + a];
    for (int b = 0; b < ynbf; ++b) {
      const uint32_t yc = ys.bpf_code[ybf + b];
      const double cc = cx * (double)ys.bpf_p[ybf + b];
      v[0] += co[xc * 16u + yc] * cc;
      if (NP == 2) {
        v[2] += dco[xc * 16u + yc] * cc;
      } else {
        v[2] += xc == yc ? cc : 0.0;
        v[3] += xc == yc ? 0.0 : cc;
      }
    }
  }
  const double tx = yw * x_nbp / x_nseq, ty = xw * y_nbp / y_nseq;
  v[0] += gap2 * tx;
  v[0] += gap2 * ty;
  v[1] = dgap2 * tx + dgap2 * ty;
}

// One pair: k[0] the value, k[1 + p] the tangents, the lanes' shares summed.
template <int NP>
__device__ void grad_pair(const StemGradLaunch& P, double* __restrict__ S, double* __restrict__ G,
                          double* __restrict__ slab, int x, int y, int lane, double* k) {
  constexpr int T = 1 + NP;
  const DevSet& s = P.xset;
  const DevSet& ys = P.yset;
#pragma unroll
  for (int c = 0; c < T; ++c) k[c] = 0.0;
  const int nlx = s.ex_nl[x], nly = ys.ex_nl[y];
  if (nlx == 0 || nly == 0) return;
  const double* __restrict__ gp = P.gpow;
  const double* __restrict__ dgp = P.dgpow;
  const double* __restrict__ co = P.co;
  const double* __restrict__ dco = P.dco;
  const int64_t stride = P.stride;
  const int64_t rowd = (int64_t)T * stride;  // a slab row: T components
  const double gap2 = P.gap2, dgap2 = P.dgap2;
  const int band = (int)P.band;
  const int xnb = s.ex_node_base[x], xbb = s.ex_bpf_base[x];
  const double x_nseq = (double)s.ex_nseqs[x];
  int chp = s.ex_xch_base[x];
  const int ynb = ys.ex_node_base[y], yeb = ys.ex_edge_base[y], ybb = ys.ex_bpf_base[y];
  const int32_t* __restrict__ ylv = ys.lvl + ys.ex_lvl_base[y];
  const int nlev = ys.ex_nlev[y];
  const double y_nseq = (double)ys.ex_nseqs[y];

  for (int r = 0; r < nlx; ++r) {
    const XRow xr = s.xrow[xnb + r];
    const int xne = xr.a & 0xff, xnbf = (xr.a >> 8) & 0xff;
    const bool xloop = xne == 0;
    const double xeg0 = gp[xr.a >> 16], dxeg0 = dgp[xr.a >> 16];
    const int xlen = xr.b & 0xffff;
    const uint32_t pslot = xr.b >> 16;
    const int xbf = xbb + (int)(xr.c & 0xffff);
    const double xw = (double)xr.w;
    const double xwg = gap2 * xw, dxwg = dgap2 * xw;
    const double x_nbp = (double)xr.nbp;
    const double xSL = P.xr_SL[xnb + r], dxSL = P.xr_dSL[xnb + r];

    // ---- A: weighted child-row sum (x loop rows have only a leaf child: S = 0)
    for (int q = lane; q < nly; q += 64) {
      double acc[T];
#pragma unroll
      for (int c = 0; c < T; ++c) acc[c] = 0.0;
      for (int t = 0; t < xne; ++t) {
        const uint32_t ch = s.xr_ch[chp + t];
        const double* row = slab + (int64_t)(ch & 0xffff) * rowd + q;
        const double w = gp[ch >> 16], dw = dgp[ch >> 16];
        const double g0 = row[0];
        acc[0] += w * g0;
        acc[1] += dw * g0 + w * row[stride];
#pragma unroll
        for (int c = 2; c < T; ++c) acc[c] += w * row[c * stride];
      }
#pragma unroll
      for (int c = 0; c < T; ++c) S[c * stride + q] = acc[c];
    }
    chp += xne;
    grad_lane_exchange_fence();

    // ---- B: MATCH and IY, level by level
    double rowk[T];
#pragma unroll
    for (int c = 0; c < T; ++c) rowk[c] = 0.0;
    for (int lv = 0; lv < nlev; ++lv) {
      const int q1 = ylv[lv + 1];
      for (int q = ylv[lv] + lane; q < q1; q += 64) {
        const uint32_t a = ys.nd_a[ynb + q];
        const int ne = (a >> 16) & 0xff, e0 = a & 0xffff, ynbf = a >> 24;
        const uint32_t b = ys.nd_b[ynb + q];
        const int ylen = b & 0xffff;
        const double wy = (double)ys.nd_w[ynb + q];
        double M[T];
#pragma unroll
        for (int c = 0; c < T; ++c) M[c] = 0.0;
        if (band == 0 || abs(xlen - ylen) <= band) {
          double H[T];
#pragma unroll
          for (int c = 0; c < T; ++c) H[c] = 0.0;
          if (ne == 0) {  // loop node: its single leaf child, G0[*][leaf] closed form
            const uint32_t g = ys.nd_c[ynb + q];
            const double f = xloop ? xeg0 : xSL, df = xloop ? dxeg0 : dxSL;
            H[0] = f * gp[g];
            H[1] = df * gp[g] + f * dgp[g];
          } else if (!xloop) {
            for (int t = 0; t < ne; ++t) {
              const uint32_t e = ys.ed[yeb + e0 + t].x;
              const double w = gp[e >> 16], dw = dgp[e >> 16];
              const double* sq = S + (e & 0xffff);
              const double s0 = sq[0];
              H[0] += w * s0;
              H[1] += dw * s0 + w * sq[stride];
#pragma unroll
              for (int c = 2; c < T; ++c) H[c] += w * sq[c * stride];
            }
          }
          bool any = false;
#pragma unroll
          for (int c = 0; c < T; ++c) any = any || H[c] != 0.0;
          if (any) {
            double v[T];
            grad_node_score<NP>(v, co, dco, s, xbf, xnbf, x_nbp, x_nseq, xw, ys, ybb + (int)(b >> 16), ynbf,
                                (double)ys.nd_nbp[ynb + q], y_nseq, wy, gap2, dgap2);
            M[0] = v[0] * H[0];
#pragma unroll
            for (int c = 1; c < T; ++c) M[c] = v[c] * H[0] + v[0] * H[c];
          }
        }
        double g1[T];
#pragma unroll
        for (int c = 0; c < T; ++c) g1[c] = M[c];
        if (ne > 0) {  // G1[q] += G1[cy] * v_s * e_s  (stem_kernel.cpp:61-77 order)
          const double vsy = gap2 * wy, dvsy = dgap2 * wy;
          for (int t = 0; t < ne; ++t) {
            const uint32_t e = ys.ed[yeb + e0 + t].x;
            const double w = gp[e >> 16], dw = dgp[e >> 16];
            const double* gq = G + (e & 0xffff);
            const double c0 = gq[0];
            g1[0] += c0 * vsy * w;
            g1[1] += (gq[stride] * vsy + c0 * dvsy) * w + c0 * vsy * dw;
#pragma unroll
            for (int c = 2; c < T; ++c) g1[c] += gq[c * stride] * vsy * w;
          }
        }
        const double py = ys.nd_P[ynb + q];
#pragma unroll
        for (int c = 0; c < T; ++c) {
          G[c * stride + q] = g1[c];
          rowk[c] += M[c] * py;
        }
      }
      grad_lane_exchange_fence();
    }
#pragma unroll
    for (int c = 0; c < T; ++c) k[c] += xr.P * rowk[c];

    // ---- C: G0 row p (rows nobody reads are not stored)
    if (pslot != 0xffffu) {
      double* orow = slab + (int64_t)pslot * rowd;
      for (int q = lane; q < nly; q += 64) {
        const double s0 = S[q];
        orow[q] = G[q] + xwg * s0;
        orow[stride + q] = G[stride + q] + (dxwg * s0 + xwg * S[stride + q]);
#pragma unroll
        for (int c = 2; c < T; ++c) orow[c * stride + q] = G[c * stride + q] + xwg * S[c * stride + q];
      }
    }
    grad_lane_exchange_fence();
  }
#pragma unroll
  for (int c = 0; c < T; ++c)
    for (int off = 32; off > 0; off >>= 1) k[c] += __shfl_xor(k[c], off, 64);
}

template <int NP>
__global__ void __launch_bounds__(64 * kStemGradWaves) sk_stem_grad_kernel(StemGradLaunch P) {
  constexpr int T = 1 + NP;
  const int lane = threadIdx.x & 63;
  // wave index as an SGPR value: the pair loop and everything in grad_pair
  // that depends on the pair is wave-uniform
  const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kStemGradWaves + (threadIdx.x >> 6)));
  const int nw = (int)gridDim.x * kStemGradWaves;
  double* base = P.scratch + (int64_t)gw * P.wave_doubles;
  double* S = base;
  double* G = base + (int64_t)T * P.stride;
  double* slab = base + (int64_t)2 * T * P.stride;
  // pairs dealt cyclically (the host orders them costliest first)
  for (int64_t k = gw; k < P.n_pairs; k += nw) {
    double v[T];
    grad_pair<NP>(P, S, G, slab, P.xs[k], P.ys[k], lane, v);
    if (lane == 0) {
      const int64_t o = P.oidx[k];
      P.value[o] = v[0];
      double* g = P.grad + 4 * o;
      g[0] = v[1];
      if (NP == 2) {
        g[1] = v[2];
        g[2] = 0.0;
        g[3] = 0.0;
      } else {
        g[1] = 0.0;
        g[2] = v[2];
        g[3] = v[3];
      }
    }
  }
}

}  // namespace

hipError_t launch_stem_grad_prep(const StemGradPrep& P, hipStream_t st) {
  if (P.s.n_examples <= 0) return hipSuccess;
  const int bs = 64;
  const int grid = (P.s.n_examples + bs - 1) / bs;
  hipLaunchKernelGGL(sk_stem_grad_prep_kernel, dim3(grid), dim3(bs), 0, st, P);
  return hipGetLastError();
}

hipError_t launch_stem_grad(const StemGradLaunch& P, bool subst, int grid, hipStream_t st) {
  if (grid <= 0 || P.n_pairs <= 0) return hipSuccess;
  if (subst)
    hipLaunchKernelGGL(sk_stem_grad_kernel<2>, dim3(grid), dim3(64 * kStemGradWaves), 0, st, P);
  else
    hipLaunchKernelGGL(sk_stem_grad_kernel<3>, dim3(grid), dim3(64 * kStemGradWaves), 0, st, P);
  return hipGetLastError();
}

}  // namespace sk
