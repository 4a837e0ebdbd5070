// Consensus (alifold-style) partition function of an alignment on CDNA4
// (gfx950): base-pairing probabilities of alignment COLUMNS, the reference's
// BPMatrix ALIFOLD (common/bpmatrix.cpp:355-397, ViennaRNA's pf_alifold; not
// in this image -- the model is DESIGN.md §9's, parity unpinned like the
// single-sequence fold's).
//
// A consensus structure sigma over the n columns of S rows weighs
//   exp(-(sum_s E_s(sigma) - sum_{(i,j) in sigma} pscore(i,j)) / (S kT)),
// E_s the single-sequence loop model (fold.hip) on row s with loop sizes in
// columns and a row's non-pairing columns read as a pair of no stacking
// energy that pays the terminal penalty.  Every loop term that does not
// depend on the row (hairpin, bulge >= 2, interior, Ninio, multiloop) keeps
// the fold's Boltzmann factor: S rows of E over S kT.  What depends on the
// rows factors into per-cell tables, written by a first phase:
//   A(i,j)   = exp(-m(i,j) TerminalAU / T), m = rows whose type pays it, T = S kT
//   CAA(i,j) = allowed ? exp(pscore / T) A^2 : 0
//   S0c, S1c, S2c(i,j) = exp(-sum_s stack / T) / (A(i,j) A(inner)) for the
//     inner pairs (i+1,j-1), (i+2,j-1), (i+1,j-2); the two bulges carry bulge(1)
// and the passes run over B = Qb A: every use of Qb outside a stack carries
// A(inner) (interior loops, multiloop and exterior branches), and a stack is
// B(inner) S0c A(i,j).  So
//   B(i,j) = CAA(i,j) [hairpin + sum B(p,q) F(n1,n2) + multiloop],
// F the fold's bulge / interior factor, S0c / S1c / S2c for the three
// row-dependent loops: the inner loops are the fold's without its pair-type
// lookups.  The outside pass keeps G = dZ/d[...] = (dZ/dB) CAA per cell;
// P(i,j) = B dZ/dB / Z.  Tables by diagonal, teams, the LDS ring and the
// per-nucleotide scale as in fold.hip.
#include <hip/hip_runtime.h>

#include "fold_dev.h"
#include "launch.h"

namespace sk {

template <bool RING>
__global__ void __launch_bounds__(512) sk_fold_ali_kernel(FoldAliLaunch P) {
  extern __shared__ __attribute__((aligned(16))) double fsm[];
  __shared__ double red[8];
  const FoldAliSeq sq = P.alns[blockIdx.x];
  const int n = sq.n, S = sq.n_rows;
  const int tid = threadIdx.x, nt = blockDim.x;
  const size_t N2 = (size_t)n * n;
  double* W = P.F.work + sq.work_off;
  double *B = W, *Qm = W + N2, *Qm1 = W + 2 * N2, *Gt = W + 3 * N2, *Hm = W + 4 * N2, *Hm1 = W + 5 * N2;
  double *CAA = W + 6 * N2, *S0c = W + 7 * N2, *S1c = W + 8 * N2, *S2c = W + 9 * N2;
  double *Q5 = W + 10 * N2, *H5 = Q5 + n + 1;
  // LDS: the Boltzmann tables, the ring (RING)
  double* tl = fsm;
  double* ring = tl + P.F.n_tab_pad;
  for (int k = tid; k < P.F.n_tab; k += nt) tl[k] = P.F.tab[k];
  __syncthreads();
  const double *bu = tl + P.F.o_bu, *in = tl + P.F.o_in, *ni = tl + P.F.o_ni, *hp = tl + P.F.o_hp;
  const double* scp = tl + P.F.o_scp;
  const double mlc = tl[P.F.o_ml], mli = tl[P.F.o_ml + 1];
  auto D = [&](int d, int i) { return (size_t)d * n + i; };
  auto slot = [](int d) { return d % kFoldRing; };
  auto dn = [](int sl) { return sl == 0 ? kFoldRing - 1 : sl - 1; };
  auto up = [](int sl) { return sl == kFoldRing - 1 ? 0 : sl + 1; };
  // bulge / interior factor of the loops whose energy the rows share
  auto loopf = [&](int n1, int n2) { return (n1 == 0 || n2 == 0) ? bu[n1 + n2] : in[n1 + n2] * ni[abs(n1 - n2)]; };
  // first n2 of the shared-energy loops at n1 (the stack and the 1-nucleotide bulges are per row)
  auto n2_first = [](int n1) { return n1 == 0 ? 2 : (n1 == 1 ? 1 : 0); };

  // ---------------------------------------------------------------- per-cell tables
  {
    const double* est = tl + P.o_ali;
    const double T = (double)S * est[64], tau = est[65], bulge1 = (double)S * est[66];
    const int8_t* rc = P.codes + sq.row_off;
    const uint8_t* __restrict__ lp = P.F.lp ? P.F.lp + sq.lp_off : nullptr;
    const bool ngu = P.F.no_gu != 0;
    for (size_t idx = tid; idx < N2; idx += nt) {
      const int d = (int)(idx / n), i = (int)(idx - (size_t)d * n);
      if (d < 4 || i >= n - d) continue;
      const int j = i + d;
      AliCounts pf;
      int m = 0, m11 = 0, m21 = 0, m12 = 0;
      double e0 = 0.0, e1 = 0.0, e2 = 0.0;  // sums of dcal/mol integers: exact
      for (int s = 0; s < S; ++s) {
        const int8_t* c = rc + (size_t)s * n;
        const int t = ali_row_type(c[i], c[j], ngu);
        pf.add(t);
        const int e = ali_energy_type(t);
        const int ea = ali_energy_type(ali_row_type(c[i + 1], c[j - 1], ngu));
        const int eb = ali_energy_type(ali_row_type(c[i + 2], c[j - 1], ngu));
        const int ec = ali_energy_type(ali_row_type(c[i + 1], c[j - 2], ngu));
        m += e > 2;
        m11 += ea > 2;
        m21 += eb > 2;
        m12 += ec > 2;
        e0 += est[e * 8 + ali_reversed(ea)];
        e1 += est[e * 8 + ali_reversed(eb)];
        e2 += est[e * 8 + ali_reversed(ec)];
      }
      int64_t ps = 0;
      const bool ok = ali_allowed(pf, S, d, &ps) && (!lp || lp[(size_t)i * n + j]);
      CAA[idx] = ok ? exp(((double)ps - 2.0 * m * tau) / T) : 0.0;
      S0c[idx] = exp(-(e0 - (m + m11) * tau) / T);
      S1c[idx] = exp(-(bulge1 + e1 - (m + m21) * tau) / T);
      S2c[idx] = exp(-(bulge1 + e2 - (m + m12) * tau) / T);
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- inside
  for (int d = 4; d < n; ++d) {
    const int ncell = n - d;
    const int G = team_of(ncell, nt);
    for (int base = 0; base < ncell; base += nt / G) {
      const int i0 = base + tid / G, r = tid % G;
      const bool on = i0 < ncell;
      const int i = on ? i0 : 0, j = i + d;
      const double caa = on ? CAA[D(d, i)] : 0.0;
      double part = 0.0;
      if (caa != 0.0) {
        // loops closed inside by (p, q) = (i+1+n1, j-1-n2), n1 + n2 <= 30,
        // q >= p + 4: diagonal d-2-n1-n2
        for (int n1 = r; n1 <= min(30, d - 6); n1 += G) {
          const int p = i + 1 + n1;
          const int n2m = min(30 - n1, d - 6 - n1);
          const int n2s = n2_first(n1);
          int sl = slot(d - 2 - n1 - n2s);
          for (int n2 = n2s; n2 <= n2m; ++n2) {
            const double v = RING ? ring[(size_t)sl * P.F.ring_n + p] : B[D(d - 2 - n1 - n2, p)];
            sl = dn(sl);
            if (v != 0.0) part += v * loopf(n1, n2) * scp[n1 + n2 + 2];
          }
        }
        if (r == 0) {  // the stack and the two 1-nucleotide bulges
          auto Bd = [&](int dd, int p) { return RING ? ring[(size_t)slot(dd) * P.F.ring_n + p] : B[D(dd, p)]; };
          if (d >= 6) part += Bd(d - 2, i + 1) * S0c[D(d, i)] * scp[2];
          if (d >= 7) part += (Bd(d - 3, i + 2) * S1c[D(d, i)] + Bd(d - 3, i + 1) * S2c[D(d, i)]) * scp[3];
        }
        // multiloop closed by (i, j): Qm(i+1, u) Qm1(u+1, j-1), u = i+e
        double ml = 0.0;
#pragma unroll 4
        for (int e = 5 + r; e + 6 <= d; e += G) ml += Qm[D(e - 1, i + 1)] * Qm1[D(d - e - 2, i + e + 1)];
        part += ml * mlc * scp[2];
      }
      part = team_sum(part, G);
      const double qb = caa != 0.0 ? caa * (hp[d - 1] * scp[d + 1] + part) : 0.0;
      if (on && r == 0) {
        B[D(d, i)] = qb;
        if (RING) ring[(size_t)slot(d) * P.F.ring_n + i] = qb;
      }
      double m1 = 0.0;  // Qm1(i, j): B(i, l) closing the branch, l = i+4 .. j
      if (on) {
#pragma unroll 4
        for (int l = i + 4 + r; l <= j; l += G) {
          const double v = l == j ? qb : B[D(l - i, i)];
          if (v != 0.0) m1 += v * mli * scp[j - l];
        }
      }
      m1 = team_sum(m1, G);
      if (on && r == 0) Qm1[D(d, i)] = m1;
      double m = 0.0;  // Qm(i, j) = sum_u (sc^(u-i) + Qm(i, u-1)) Qm1(u, j)
      if (on) {
#pragma unroll 4
        for (int u = i + r; u + 4 <= j; u += G)
          m += (scp[u - i] + (u - 1 >= i ? Qm[D(u - 1 - i, i)] : 0.0)) * (u == i ? m1 : Qm1[D(j - u, u)]);
      }
      m = team_sum(m, G);
      if (on && r == 0) Qm[D(d, i)] = m;
    }
    __syncthreads();
  }

  // ---------------------------------------------------------------- exterior
  if (tid == 0) Q5[0] = 1.0;
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    double s = 0.0;
    for (int k = tid; k + 4 <= j; k += nt) s += Q5[k] * B[D(j - k, k)];
    s = block_sum(s, red);
    if (tid == 0) Q5[j + 1] = Q5[j] * scp[1] + s;
    __syncthreads();
  }
  const double Z = Q5[n];
  if (tid == 0 && P.F.log_z) P.F.log_z[blockIdx.x] = log(Z) - (double)n * P.F.log_sc;
  if (tid == 0) H5[n] = 1.0;
  __syncthreads();
  for (int k = n - 1; k >= 0; --k) {
    double s = 0.0;
    for (int j = k + 4 + tid; j < n; j += nt) s += H5[j + 1] * B[D(j - k, k)];
    s = block_sum(s, red);
    if (tid == 0) H5[k] = H5[k + 1] * scp[1] + s;
    __syncthreads();
  }

  // ---------------------------------------------------------------- outside
  // (the ring now holds the G diagonals above the span: every one read was
  // written by an earlier span of this pass)
  double* __restrict__ out = P.F.out + sq.out_off;
  for (int d = n - 1; d >= 4; --d) {
    const int ncell = n - d;
    const int G = team_of(ncell, nt);
    for (int base = 0; base < ncell; base += nt / G) {
      const int i0 = base + tid / G, r = tid % G;
      const bool on = i0 < ncell;
      const int i = on ? i0 : 0, j = i + d;
      // Hm(i,j): Qm(i,j2) += Qm(i,j) Qm1(j+1,j2);  B(i-1,j') ML rule with u = j
      double hm = 0.0;
      if (on) {
#pragma unroll 4
        for (int j2 = j + 5 + r; j2 < n; j2 += G) hm += Hm[D(j2 - i, i)] * Qm1[D(j2 - j - 1, j + 1)];
        if (i >= 1) {
          for (int jp = j + 6 + r; jp < n; jp += G) {
            const double v = Gt[D(jp - i + 1, i - 1)];
            if (v != 0.0) hm += v * mlc * scp[2] * Qm1[D(jp - j - 2, j + 1)];
          }
        }
      }
      hm = team_sum(hm, G);
      if (on && r == 0) Hm[D(d, i)] = hm;
      // Hm1(i,j): Qm(ii,j) += (sc^(i-ii) + Qm(ii,i-1)) Qm1(i,j), ii <= i;
      //           B(i',j+1) ML rule with u + 1 = i
      double hm1 = 0.0;
      if (on) {
#pragma unroll 4
        for (int e = r; e <= i; e += G) {
          const double v = e == 0 ? hm : Hm[D(d + e, i - e)];
          if (v != 0.0) hm1 += v * (scp[e] + (e >= 1 ? Qm[D(e - 1, i - e)] : 0.0));
        }
        if (j + 1 < n) {
          for (int e = 6 + r; e <= i; e += G) {  // ip = i - e
            const double v = Gt[D(d + 1 + e, i - e)];
            if (v != 0.0) hm1 += v * mlc * scp[2] * Qm[D(e - 2, i - e + 1)];
          }
        }
      }
      hm1 = team_sum(hm1, G);
      if (on && r == 0) Hm1[D(d, i)] = hm1;
      // dZ/dB(i,j): exterior branch, Qm1(i,jj) += B(i,j) (branch) sc^(jj-j),
      //             enclosing loops (ip, jp) = (i-1-n1, j+1+n2): diagonal d+2+n1+n2
      const double caa = on ? CAA[D(d, i)] : 0.0;
      double part = 0.0;
      if (caa != 0.0) {
        double s = r == 0 ? hm1 : 0.0;
#pragma unroll 4
        for (int jj = j + 1 + r; jj < n; jj += G) s += Hm1[D(jj - i, i)] * scp[jj - j];
        part = s * mli;
        for (int n1 = r; n1 <= min(30, i - 1); n1 += G) {
          const int ip = i - 1 - n1;
          const int n2m = min(30 - n1, n - 2 - j);
          const int n2s = n2_first(n1);
          int sl = slot(d + 2 + n1 + n2s);
          for (int n2 = n2s; n2 <= n2m; ++n2) {
            const double v = RING ? ring[(size_t)sl * P.F.ring_n + ip] : Gt[D(d + 2 + n1 + n2, ip)];
            sl = up(sl);
            if (v != 0.0) part += v * loopf(n1, n2) * scp[n1 + n2 + 2];
          }
        }
        if (r == 0) {  // (i, j) stacked on, or a 1-nucleotide bulge inside, its enclosing pair
          auto Gd = [&](int dd, int p) { return RING ? ring[(size_t)slot(dd) * P.F.ring_n + p] : Gt[D(dd, p)]; };
          if (i >= 1 && j + 1 < n) part += Gd(d + 2, i - 1) * S0c[D(d + 2, i - 1)] * scp[2];
          if (i >= 2 && j + 1 < n) part += Gd(d + 3, i - 2) * S1c[D(d + 3, i - 2)] * scp[3];
          if (i >= 1 && j + 2 < n) part += Gd(d + 3, i - 1) * S2c[D(d + 3, i - 1)] * scp[3];
        }
      }
      part = team_sum(part, G);
      if (on && r == 0) {
        const double gb = caa != 0.0 ? H5[j + 1] * Q5[i] + part : 0.0;
        const double g = gb * caa;
        Gt[D(d, i)] = g;
        if (RING) ring[(size_t)slot(d) * P.F.ring_n + i] = g;
        out[(size_t)i * n - (size_t)i * (i + 1) / 2 + (size_t)(j - i - 1)] = B[D(d, i)] * gb / Z;
      }
    }
    __syncthreads();
  }
}

size_t fold_ali_lds_bytes(const FoldLaunch& F, int max_n) {
  return ((size_t)F.n_tab_pad + (fold_ring(max_n) ? (size_t)kFoldRing * max_n : 0)) * 8;
}

template <bool RING>
static hipError_t launch_fold_ali_t(const FoldAliLaunch& P, int n_alns, size_t lds, hipStream_t st) {
  hipError_t e = hipFuncSetAttribute((const void*)sk_fold_ali_kernel<RING>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((sk_fold_ali_kernel<RING>), dim3(n_alns), dim3(512), lds, st, P);
  return hipGetLastError();
}

hipError_t launch_fold_ali(const FoldAliLaunch& P0, int n_alns, int max_n, hipStream_t st) {
  if (n_alns <= 0) return hipSuccess;
  FoldAliLaunch P = P0;
  P.F.ring_n = fold_ring(max_n) ? max_n : 0;
  const size_t lds = fold_ali_lds_bytes(P.F, max_n);
  if (lds > kFoldLdsMax) return hipErrorInvalidValue;
  return fold_ring(max_n) ? launch_fold_ali_t<true>(P, n_alns, lds, st) : launch_fold_ali_t<false>(P, n_alns, lds, st);
}

}  // namespace sk
