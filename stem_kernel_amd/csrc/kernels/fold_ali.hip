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
// per-nucleotide scale as in fold.hip, and the passes themselves -- Qm1, Qm,
// the Q5 / H5 sweeps, Hm, Hm1 -- are the fold's (fold_dev.h), run with a pair
// model that answers 1: here are only the per-cell phase and the loop sums
// over B and G.  Work layout: FoldWork of kFoldAliTables tables (launch.h).
#include <hip/hip_runtime.h>

#include "fold_dev.h"
#include "launch.h"

namespace sk {

// The pair model of the shared passes: CAA carries the terminal factors and
// decides which column pairs form (B and G are 0 elsewhere)
struct AliPairModel {
  __device__ __forceinline__ double branch(int, int) const { return 1.0; }
  __device__ __forceinline__ double closer(int, int) const { return 1.0; }
};

// 512 threads (8 waves; 88 VGPRs with the ring, 91 without: 5 waves per
// SIMD, no scratch)
template <bool RING>
__global__ void __launch_bounds__(512) sk_fold_ali_kernel(FoldLaunch P) {
  extern __shared__ __attribute__((aligned(16))) double fsm[];
  __shared__ double red[8];
  const FoldSeq sq = P.seqs[blockIdx.x];
  const int n = sq.n, S = sq.n_rows;
  const int tid = threadIdx.x, nt = blockDim.x;
  const FoldWork w{P.work + sq.work_off, (size_t)n, kFoldAliTables};
  enum { kCAA, kS0c, kS1c, kS2c };  // the per-cell tables; B is the passes' Qb, G their Hb
  // LDS: the Boltzmann tables, the ring (RING)
  double* tl = fsm;
  double* ring = tl + P.n_tab_pad;
  for (int k = tid; k < P.n_tab; k += nt) tl[k] = P.tab[k];
  __syncthreads();
  const FoldTables T = fold_table_views(P, tl, tl);
  const double* scp = T.scp;
  const AliPairModel M;
  // bulge / interior factor of the loops whose energy the rows share
  auto loopf = [&](int n1, int n2) {
    return (n1 == 0 || n2 == 0) ? T.bu[n1 + n2] : T.in[n1 + n2] * T.ni[abs(n1 - n2)];
  };
  // first n2 of the shared-energy loops at n1 (the stack and the 1-nucleotide bulges are per row)
  auto n2_first = [](int n1) { return n1 == 0 ? 2 : (n1 == 1 ? 1 : 0); };
  // a cell of B (inside) or G (outside) within the interior-loop window
  auto Bw = [&](int dd, int p) { return RING ? ring[(size_t)fold_ring_slot(dd) * P.max_n + p] : w.qb(dd, p); };
  auto Gw = [&](int dd, int p) { return RING ? ring[(size_t)fold_ring_slot(dd) * P.max_n + p] : w.hb(dd, p); };

  // ---------------------------------------------------------------- per-cell tables
  {
    const double* est = tl + P.o_ali;
    const double Tk = (double)S * est[64], tau = est[65], bulge1 = (double)S * est[66];
    const int8_t* rc = P.codes + sq.seq_off;
    const uint8_t* __restrict__ lp = P.lp ? P.lp + sq.lp_off : nullptr;
    const bool ngu = P.no_gu != 0;
    // (written by idx = d n + i through pointers: the accessors' address
    // arithmetic here costs scalar registers the row loop then spills)
    double *CAA = &w.cell(kCAA, 0, 0), *S0c = &w.cell(kS0c, 0, 0);
    double *S1c = &w.cell(kS1c, 0, 0), *S2c = &w.cell(kS2c, 0, 0);
    for (size_t idx = tid; idx < w.n * w.n; idx += nt) {
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
      CAA[idx] = ok ? exp(((double)ps - 2.0 * m * tau) / Tk) : 0.0;
      S0c[idx] = exp(-(e0 - (m + m11) * tau) / Tk);
      S1c[idx] = exp(-(bulge1 + e1 - (m + m21) * tau) / Tk);
      S2c[idx] = exp(-(bulge1 + e2 - (m + m12) * tau) / Tk);
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
      const double caa = on ? w.cell(kCAA, d, i) : 0.0;
      double part = 0.0;
      if (caa != 0.0) {
        // loops closed inside by (p, q) = (i+1+n1, j-1-n2), n1 + n2 <= 30,
        // q >= p + 4: diagonal d-2-n1-n2
        for (int n1 = r; n1 <= min(30, d - 6); n1 += G) {
          const int p = i + 1 + n1;
          const int n2m = min(30 - n1, d - 6 - n1);
          const int n2s = n2_first(n1);
          int sl = fold_ring_slot(d - 2 - n1 - n2s);
          for (int n2 = n2s; n2 <= n2m; ++n2) {
            const double v = RING ? ring[(size_t)sl * P.max_n + p] : w.qb(d - 2 - n1 - n2, p);
            sl = fold_ring_dn(sl);
            if (v != 0.0) part += v * loopf(n1, n2) * scp[n1 + n2 + 2];
          }
        }
        if (r == 0) {  // the stack and the two 1-nucleotide bulges
          if (d >= 6) part += Bw(d - 2, i + 1) * w.cell(kS0c, d, i) * scp[2];
          if (d >= 7)
            part += (Bw(d - 3, i + 2) * w.cell(kS1c, d, i) + Bw(d - 3, i + 1) * w.cell(kS2c, d, i)) * scp[3];
        }
        // multiloop closed by (i, j): Qm(i+1, u) Qm1(u+1, j-1), u = i+e
        double ml = 0.0;
#pragma unroll 4
        for (int e = 5 + r; e + 6 <= d; e += G) ml += w.qm(e - 1, i + 1) * w.qm1(d - e - 2, i + e + 1);
        part += ml * T.mlc * scp[2];
      }
      part = team_sum(part, G);
      const double qb = caa != 0.0 ? caa * (T.hp[d - 1] * scp[d + 1] + part) : 0.0;
      if (on && r == 0) {
        w.qb(d, i) = qb;
        if (RING) ring[(size_t)fold_ring_slot(d) * P.max_n + i] = qb;
      }
      fold_qm_updates(w, T, M, i, j, r, G, on, qb);
    }
    __syncthreads();
  }

  // ---------------------------------------------------------------- exterior
  const double Z = fold_q5_sweep(w, T, M, red);
  if (tid == 0 && P.log_z) P.log_z[blockIdx.x] = log(Z) - (double)n * P.log_sc;
  fold_h5_sweep(w, T, M, red);

  // ---------------------------------------------------------------- outside
  // (the ring now holds the G diagonals above the span: every one read was
  // written by an earlier span of this pass)
  double* __restrict__ out = P.out + sq.out_off;
  for (int d = n - 1; d >= 4; --d) {
    const int ncell = n - d;
    const int G = team_of(ncell, nt);
    for (int base = 0; base < ncell; base += nt / G) {
      const int i0 = base + tid / G, r = tid % G;
      const bool on = i0 < ncell;
      const int i = on ? i0 : 0, j = i + d;
      const double hm1 = fold_hm_updates(w, T, M, i, j, r, G, on);
      // dZ/dB(i,j): exterior branch, Qm1(i,jj) += B(i,j) (branch) sc^(jj-j),
      //             enclosing loops (ip, jp) = (i-1-n1, j+1+n2): diagonal d+2+n1+n2
      const double caa = on ? w.cell(kCAA, d, i) : 0.0;
      double part = 0.0;
      if (caa != 0.0) {
        double s = r == 0 ? hm1 : 0.0;
#pragma unroll 4
        for (int jj = j + 1 + r; jj < n; jj += G) s += w.hm1(jj - i, i) * scp[jj - j];
        part = s * T.mli;
        for (int n1 = r; n1 <= min(30, i - 1); n1 += G) {
          const int ip = i - 1 - n1;
          const int n2m = min(30 - n1, n - 2 - j);
          const int n2s = n2_first(n1);
          int sl = fold_ring_slot(d + 2 + n1 + n2s);
          for (int n2 = n2s; n2 <= n2m; ++n2) {
            const double v = RING ? ring[(size_t)sl * P.max_n + ip] : w.hb(d + 2 + n1 + n2, ip);
            sl = fold_ring_up(sl);
            if (v != 0.0) part += v * loopf(n1, n2) * scp[n1 + n2 + 2];
          }
        }
        if (r == 0) {  // (i, j) stacked on, or a 1-nucleotide bulge inside, its enclosing pair
          if (i >= 1 && j + 1 < n) part += Gw(d + 2, i - 1) * w.cell(kS0c, d + 2, i - 1) * scp[2];
          if (i >= 2 && j + 1 < n) part += Gw(d + 3, i - 2) * w.cell(kS1c, d + 3, i - 2) * scp[3];
          if (i >= 1 && j + 2 < n) part += Gw(d + 3, i - 1) * w.cell(kS2c, d + 3, i - 1) * scp[3];
        }
      }
      part = team_sum(part, G);
      if (on && r == 0) {
        const double gb = caa != 0.0 ? w.h5()[j + 1] * w.q5()[i] + part : 0.0;
        const double g = gb * caa;
        w.hb(d, i) = g;
        if (RING) ring[(size_t)fold_ring_slot(d) * P.max_n + i] = g;
        out[tri_index(n, i, j)] = w.qb(d, i) * gb / Z;
      }
    }
    __syncthreads();
  }
}

FoldPath fold_ali_path(const FoldLaunch& P, int max_n) {
  return max_n <= kFoldRingMaxN && P.min_path != kFoldPathHbm ? kFoldPathRing : kFoldPathHbm;
}

size_t fold_ali_lds_bytes(const FoldLaunch& P, int max_n) {
  const bool ring = fold_ali_path(P, max_n) == kFoldPathRing;
  return ((size_t)P.n_tab_pad + (ring ? (size_t)kFoldRing * max_n : 0)) * 8;
}

hipError_t launch_fold_ali(const FoldLaunch& P0, int n_alns, int max_n, hipStream_t st) {
  if (n_alns <= 0) return hipSuccess;
  FoldLaunch P = P0;
  P.max_n = max_n;
  const size_t lds = fold_ali_lds_bytes(P, max_n);
  if (lds > kFoldLdsMax) return hipErrorInvalidValue;
  const bool ring = fold_ali_path(P, max_n) == kFoldPathRing;
  return launch_fold_kernel(ring ? sk_fold_ali_kernel<true> : sk_fold_ali_kernel<false>, P, dim3(n_alns), 512, lds,
                            st);
}

}  // namespace sk
