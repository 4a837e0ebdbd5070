// McCaskill base-pairing probabilities on CDNA4 (gfx950): SURVEY.md §8 f1.
//
// Replaces ViennaRNA's pf_fold as the reference calls it for every example
// (BPMatrix FOLD, common/bpmatrix.cpp:151-177; PFWrapper::fold,
// common/pf_wrapper.cpp:15-36; twice per pair in stem_kernel/stem_kernel.cpp:290-291).
// ViennaRNA and its parameter files are not in this image: the loop model is
// the Turner-1999 core the legacy library compiles in (stacks, hairpin /
// bulge / interior initiation, Ninio asymmetry, terminal AU/GU, linear
// multiloop) without its mismatch, dangle and special-loop tables
// (parity against ViennaRNA unpinned, the recursions pinned by
// exhaustive enumeration in oracle/fold_oracle.c).
//
// One workgroup per sequence.  Inside tables Qb (pair closes a loop), Qm1
// (one multiloop branch starting at i), Qm (>= 1 branch) and the exterior
// prefix Q5; outside values as adjoints of the inside rules (Hb, Hm1, Hm,
// H5), each cell PULLING from larger spans, so a span's cells are
// independent: one thread per cell, a barrier per span.  Tables are n x n
// doubles in HBM (L2-resident for n up to ~250), with transposed copies of
// the ones read down a column.  All quantities of a subsequence carry a
// per-nucleotide scale sc^len (Vienna's pf_scale), so Z stays in range for
// n up to ~1,400; P(i,j) = Qb Hb / Z is scale-free.
//
// The passes the consensus fold (fold_ali.hip) runs too -- Qm1, Qm, the Q5 /
// H5 sweeps, Hm, Hm1 -- the ring slots and the launch wrapper are in
// fold_dev.h, the work-buffer layout and its cells (FoldWork) in launch.h;
// here are the interior-loop sums and this fold's pair model (FoldPairModel).
#include <hip/hip_runtime.h>

#include "fold_dev.h"
#include "launch.h"

namespace sk {

// Tables are stored by DIAGONAL: cell (i, i+d) of a table at d*n + i.  A
// span's cells are the threads (consecutive i), and every read of a loop
// iteration sits at a fixed offset from the cell -- (i+a, j-b) lies on
// diagonal d-a-b at index i+a -- so the threads of a wave read consecutive
// doubles: coalesced, where the row-major tables gave each thread its own
// row (one cache line per lane per iteration).  The interior-loop windows
// (the 31 diagonals below the span inside, above it outside) are also kept
// in an LDS ring of kFoldRing diagonals when the sequences are short enough
// (RING: 33 n doubles), and the Boltzmann tables and the codes sit in LDS.

// 512 threads (8 waves; 100 VGPRs with the ring, 104 with the tables in HBM,
// 108 with neither: 4 waves per SIMD, no scratch; two workgroups per CU by
// LDS at L = 200)
// GTAB: the hairpin and scale tables (the tail of P.tab, sized by the
// batch's longest sequence) are read from HBM, only the fixed-size head sits
// in LDS -- long sequences, whose tables would not fit beside the codes
template <bool RING, bool GTAB>
__global__ void __launch_bounds__(512) sk_fold_kernel(FoldLaunch P) {
  extern __shared__ __attribute__((aligned(16))) double fsm[];
  __shared__ double red[8];
  const FoldSeq sq = P.seqs[blockIdx.x];
  const int n = sq.n;
  const int tid = threadIdx.x, nt = blockDim.x;
  const FoldWork w{P.work + sq.work_off, (size_t)n, kFoldTables};
  // LDS: the Boltzmann tables, the ring (RING), the codes
  double* tl = fsm;
  const int n_lds = GTAB ? P.n_small : P.n_tab;  // table entries copied to LDS
  double* ring = tl + ((n_lds + 1) & ~1);
  int8_t* c = reinterpret_cast<int8_t*>(ring + (RING ? kFoldRing * P.max_n : 0));
  for (int k = tid; k < n_lds; k += nt) tl[k] = P.tab[k];
  for (int k = tid; k < n; k += nt) c[k] = P.codes[sq.seq_off + k];
  __syncthreads();
  const FoldTables T = fold_table_views(P, tl, GTAB ? P.tab : tl);
  const double* scp = T.scp;
  const bool ncg = P.no_closing_gu != 0;
  const FoldPairModel M{c, P.lp ? P.lp + sq.lp_off : nullptr, T.au, n, P.no_gu != 0, ncg};
#ifdef SK_FOLD_TIMING  // diagnostic build: cycles per pass, printed for blocks 0 and 1
  const uint64_t tk0 = clock64();
#endif

  // ---------------------------------------------------------------- inside
  // A span's cells go to TEAMS of G lanes (team_of: as many as the block's
  // threads allow, up to 8 -- the long spans, with the most work per cell,
  // have the fewest cells): lane r of a team takes every G-th iteration of
  // each sum, and the team adds its partial sums by a butterfly (the same
  // fixed order for every cell).
  for (int d = 4; d < n; ++d) {
    const int ncell = n - d;
    const int G = team_of(ncell, nt);
    for (int base = 0; base < ncell; base += nt / G) {
      const int i0 = base + tid / G, r = tid % G;
      const bool on = i0 < ncell;
      const int i = on ? i0 : 0, j = i + d;
      const int t = on ? M.ptype(i, j) : 0;
      double part = 0.0;
      if (t) {
        // interior loops closed by (p, q) = (i+1+n1, j-1-n2), n1 + n2 <= 30,
        // q >= p + 4: diagonal d-2-n1-n2
        for (int n1 = r; n1 <= min(30, d - 6); n1 += G) {
          const int p = i + 1 + n1;
          const int n2m = min(30 - n1, d - 6 - n1);
          const int cp = c[p];
          int sl = fold_ring_slot(d - 2 - n1);
          for (int n2 = 0; n2 <= n2m; ++n2) {
            const double v = RING ? ring[(size_t)sl * P.max_n + p] : w.qb(d - 2 - n1 - n2, p);
            sl = fold_ring_dn(sl);
            if (v != 0.0)
              part += v * fold_interior(T, t, pair_raw(c[j - 1 - n2], cp), n1, n2, ncg) * scp[n1 + n2 + 2];
          }
        }
        if (!(ncg && is_gu(t))) {
          // multiloop closed by (i, j): Qm(i+1, u) Qm1(u+1, j-1), u = i+e
          double ml = 0.0;
#pragma unroll 4
          for (int e = 5 + r; e + 6 <= d; e += G) ml += w.qm(e - 1, i + 1) * w.qm1(d - e - 2, i + e + 1);
          part += ml * T.mlc * T.au[t] * scp[2];
        }
      }
      part = team_sum(part, G);
      const double qb = t ? (!(ncg && is_gu(t)) ? T.hp[d - 1] * T.au[t] * scp[d + 1] : 0.0) + part : 0.0;
      if (on && r == 0) {
        w.qb(d, i) = qb;
        if (RING) ring[(size_t)fold_ring_slot(d) * P.max_n + i] = qb;
      }
      fold_qm_updates(w, T, M, i, j, r, G, on, qb);
    }
    __syncthreads();
  }
#ifdef SK_FOLD_TIMING
  const uint64_t tk1 = clock64();
#endif

  // ---------------------------------------------------------------- exterior
  const double Z = fold_q5_sweep(w, T, M, red);
  if (tid == 0 && P.log_z) P.log_z[blockIdx.x] = log(Z) - (double)n * P.log_sc;
  // the structure sampler (fold_sample.hip) walks Qb, Qm, Qm1 and Q5 only
  if (P.inside_only) return;
  fold_h5_sweep(w, T, M, red);
#ifdef SK_FOLD_TIMING
  const uint64_t tk2 = clock64();
#endif

  // ---------------------------------------------------------------- outside
  // (the ring now holds the Hb diagonals above the span: every one read was
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
      // Hb(i,j): exterior branch, Qm1(i,jj) += Qb(i,j) (branch) sc^(jj-j),
      //          enclosing interior loops (ip, jp) = (i-1-n1, j+1+n2):
      //          diagonal d+2+n1+n2
      const int t = on ? M.ptype(i, j) : 0;
      double part = 0.0;
      if (t) {
        double s = r == 0 ? hm1 : 0.0;
#pragma unroll 4
        for (int jj = j + 1 + r; jj < n; jj += G) s += w.hm1(jj - i, i) * scp[jj - j];
        part = s * T.mli * T.au[t];
        const int t2 = pair_raw(c[j], c[i]);
        for (int n1 = r; n1 <= min(30, i - 1); n1 += G) {
          const int ip = i - 1 - n1;
          const int n2m = min(30 - n1, n - 2 - j);
          int sl = fold_ring_slot(d + 2 + n1);
          for (int n2 = 0; n2 <= n2m; ++n2) {
            const double v = RING ? ring[(size_t)sl * P.max_n + ip] : w.hb(d + 2 + n1 + n2, ip);
            sl = fold_ring_up(sl);
            if (v == 0.0) continue;
            const int t1 = M.ptype(ip, j + 1 + n2);
            if (!t1) continue;
            part += v * fold_interior(T, t1, t2, n1, n2, ncg) * scp[n1 + n2 + 2];
          }
        }
      }
      part = team_sum(part, G);
      if (on && r == 0) {
        const double hb = t ? w.h5()[j + 1] * w.q5()[i] * T.au[t] + part : 0.0;
        const double qbij = w.qb(d, i);
        w.hb(d, i) = hb;
        if (RING) ring[(size_t)fold_ring_slot(d) * P.max_n + i] = hb;
        out[tri_index(n, i, j)] = qbij != 0.0 ? qbij * hb / Z : 0.0;
      }
    }
    __syncthreads();
  }
#ifdef SK_FOLD_TIMING
  if (tid == 0 && blockIdx.x < 2)
    printf("fold b%d n %d inside %lu exterior %lu outside %lu\n", (int)blockIdx.x, n, (unsigned long)(tk1 - tk0),
           (unsigned long)(tk2 - tk1), (unsigned long)(clock64() - tk2));
#endif
}

// the dynamic LDS of sk_fold_kernel<ring, gtab>
static size_t fold_lds_bytes_t(const FoldLaunch& P, int max_n, bool ring, bool gtab) {
  const size_t ntab = gtab ? (size_t)((P.n_small + 1) & ~1) : (size_t)P.n_tab_pad;
  return (ntab + (ring ? (size_t)kFoldRing * max_n : 0)) * 8 + (size_t)(max_n + 15) / 16 * 16;
}

bool fold_ring(const FoldLaunch& P, int max_n) { return max_n <= kFoldRingMaxN && P.min_path == kFoldPathRing; }

// (a launch with the ring has at most kFoldRingMaxN nucleotides: its tables always fit)
bool fold_gtab(const FoldLaunch& P, int max_n) {
  if (fold_ring(P, max_n)) return false;
  return P.min_path == kFoldPathGtab || fold_lds_bytes_t(P, max_n, false, false) > kFoldLdsMax;
}

FoldPath fold_path(const FoldLaunch& P, int max_n) {
  return fold_ring(P, max_n) ? kFoldPathRing : fold_gtab(P, max_n) ? kFoldPathGtab : kFoldPathHbm;
}

// one decision (fold_path) gives a launch's LDS size and its kernel
size_t fold_lds_bytes(const FoldLaunch& P, int max_n) {
  const FoldPath path = fold_path(P, max_n);
  return fold_lds_bytes_t(P, max_n, path == kFoldPathRing, path == kFoldPathGtab);
}

hipError_t launch_fold(const FoldLaunch& P0, int n_seqs, int max_n, hipStream_t st) {
  if (n_seqs <= 0) return hipSuccess;
  FoldLaunch P = P0;
  P.max_n = max_n;
  const size_t lds = fold_lds_bytes(P, max_n);
  if (lds > kFoldLdsMax) return hipErrorInvalidValue;
  const FoldPath path = fold_path(P, max_n);
  return launch_fold_kernel(path == kFoldPathRing   ? sk_fold_kernel<true, false>
                            : path == kFoldPathGtab ? sk_fold_kernel<false, true>
                                                    : sk_fold_kernel<false, false>,
                            P, dim3(n_seqs), 512, lds, st);
}

}  // namespace sk
