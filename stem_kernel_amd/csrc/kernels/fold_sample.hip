// Stochastic structure sampling on CDNA4 (gfx950): BPMatrix SFOLD,
// common/bpmatrix.cpp:179-232 (pf_fold, then n_samples x pbacktrack, bpp(i,j)
// = the fraction of samples that hold the pair).
//
// Runs after an inside_only launch of the fold kernel (fold.hip), which
// leaves the inside tables Qb, Qm, Qm1 (by diagonal) and the exterior prefix
// Q5 in the work buffer (FoldWork, launch.h; the pair types, loop factors
// and launch wrapper shared with the fold: fold_dev.h).  A structure is drawn
// by walking those tables top down: an open segment is one cell of one
// table, and the candidates of its decision are exactly the terms of the inside sum that produced the cell,
// with the same pair types, loop factors and scale powers -- so a structure
// comes out with probability exp(-E/kT) / Z whatever the per-nucleotide
// scale is.
//
//   Q5[j+1]   j unpaired                      -> Q5[j]
//             pair (k, j)                     -> Q5[k], Qb(k, j)
//   Qb(i,j)   hairpin                         -> done
//             interior / bulge / stack (p,q)  -> Qb(p, q)
//             multiloop split e               -> Qm(i+1, i+e), Qm1(i+e+1, j-1)
//   Qm(i,j)   first branch at u, left empty   -> Qm1(u, j)
//             first branch at u, left Qm      -> Qm(i, u-1), Qm1(u, j)
//   Qm1(i,j)  branch closed at l              -> Qb(i, l)
//
// One wavefront draws one structure at a time; the waves of a workgroup share
// one sequence's codes and Boltzmann tables in LDS and loop over the sample
// indices.  The lanes evaluate a decision's candidates strided by 64; the
// winner is the first candidate whose running sum exceeds r x (the sum of the
// candidates as computed here), found by a wave prefix scan and a ballot.
// Every random number is a pure function of (seed, sequence index, sample
// index, decision number): fold_rng.h.
#include <hip/hip_runtime.h>

#include "fold_dev.h"
#include "fold_rng.h"
#include "launch.h"

namespace sk {

constexpr int kSampleWaves = 4;  // waves per workgroup

// open segments of one structure: disjoint, each but the exterior one holds
// a pair of its own (>= 5 nucleotides)
__host__ __device__ inline int fold_sample_stack_cap(int n) { return n / 2 + 4; }

enum : int { kSegExt = 0, kSegB = 1, kSegM = 2, kSegM1 = 3 };

// inclusive prefix sum over the wave, in every lane (the same operations for
// every call, so the two passes of choose() add alike)
__device__ __forceinline__ double wave_scan(double v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double t = __shfl_up(v, off, 64);
    if (lane >= off) v += t;
  }
  return v;
}

// Draw one of ncand candidates with probability weight(idx) / sum: the first
// whose running sum exceeds u * sum, u in [0, 1).  Both passes add the same
// numbers in the same order, so the last running sum is the total and a
// winner exists; should a compiler ever round the two passes differently,
// the last candidate of positive weight wins.  -1: the weights sum to 0 or
// to a non-finite value.  ncand and u are wave-uniform; so is the result.
template <class F>
__device__ __forceinline__ int choose(int ncand, F weight, double u, int lane) {
  double total = 0.0;
  for (int base = 0; base < ncand; base += 64) {
    const int idx = base + lane;
    const double w = idx < ncand ? weight(idx) : 0.0;
    if (__ballot(w != 0.0) == 0) continue;
    total += __shfl(wave_scan(w, lane), 63, 64);
  }
  if (!(total > 0.0) || !(total < 1.7e308)) return -1;
  const double target = u * total;
  double run = 0.0;
  int last = -1;
  for (int base = 0; base < ncand; base += 64) {
    const int idx = base + lane;
    const double w = idx < ncand ? weight(idx) : 0.0;
    if (__ballot(w != 0.0) == 0) continue;
    const double inc = wave_scan(w, lane);
    const unsigned long long pos = __ballot(w > 0.0);
    const unsigned long long hit = __ballot(w > 0.0 && run + inc > target);
    if (hit) return base + __ffsll((long long)hit) - 1;
    if (pos) last = base + 63 - __clzll((long long)pos);
    run += __shfl(inc, 63, 64);
  }
  return last;
}

__global__ void __launch_bounds__(kSampleWaves * 64) sk_fold_sample_kernel(FoldSampleLaunch S) {
  extern __shared__ __attribute__((aligned(16))) double ssm[];
  const FoldLaunch& P = S.F;
  const FoldSeq sq = P.seqs[blockIdx.x];
  const int n = sq.n;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;
  // (the tables' bases taken once: with FoldWork's accessors in every
  // candidate, or the shared table views, the walks measured 0.9 % slower)
  const FoldWork w{P.work + sq.work_off, (size_t)n, kFoldTables};
  const double *Qb = &w.qb(0, 0), *Qm = &w.qm(0, 0), *Qm1 = &w.qm1(0, 0), *Q5 = w.q5();
  // LDS: the Boltzmann tables, a stack of open segments per wave, the codes
  double* tl = ssm;
  const int cap = fold_sample_stack_cap(P.max_n);
  int2* stack = reinterpret_cast<int2*>(tl + P.n_tab_pad) + (size_t)wave * cap;
  int8_t* c = reinterpret_cast<int8_t*>(reinterpret_cast<int2*>(tl + P.n_tab_pad) + (size_t)kSampleWaves * cap);
  for (int k = tid; k < P.n_tab; k += nt) tl[k] = P.tab[k];
  for (int k = tid; k < n; k += nt) c[k] = P.codes[sq.seq_off + k];
  __syncthreads();
  FoldTables T;
  T.st = tl + P.o_st;
  T.hp = tl + P.o_hp;
  T.bu = tl + P.o_bu;
  T.in = tl + P.o_in;
  T.ni = tl + P.o_ni;
  T.au = tl + P.o_au;
  T.scp = tl + P.o_scp;
  T.mlc = tl[P.o_ml];
  T.mli = tl[P.o_ml + 1];
  const double* scp = T.scp;
  const bool ngu = P.no_gu != 0, ncg = P.no_closing_gu != 0;
  const uint8_t* __restrict__ lp = P.lp ? P.lp + sq.lp_off : nullptr;
  auto D = [&](int d, int i) { return (size_t)d * n + i; };
  uint32_t* cnt = S.cnt + sq.out_off;
  const int max_dec = 2 * n + 2;

  for (int s = blockIdx.y * kSampleWaves + wave; s < S.n_samples; s += gridDim.y * kSampleWaves) {
    char* str = S.structs ? S.structs + ((size_t)S.n_samples * sq.seq_off + (size_t)s * n) : nullptr;
    const uint64_t stream = rng_stream(S.seed, S.seq_base + (int)blockIdx.x, s);
    int sp = 0, draws = 0, bad = 0;
    // every lane holds the same sp and writes the same entry: no lane reads
    // what another one wrote
    auto push = [&](int type, int i, int j) {
      if (sp >= cap) {
        bad = kFoldSampleStack;
        return;
      }
      stack[sp++] = make_int2(i | type << 28, j);
    };
    auto add_pair = [&](int i, int j) {
      if (lane == 0) {
        atomicAdd(&cnt[(size_t)i * n - (size_t)i * (i + 1) / 2 + (size_t)(j - i - 1)], 1u);
        if (str) {
          str[i] = '(';
          str[j] = ')';
        }
      }
    };
    if (n >= 5) push(kSegExt, 0, n);
    while (sp > 0 && !bad) {
      const int2 e = stack[--sp];
      const int type = __builtin_amdgcn_readfirstlane(e.x >> 28);
      const int i = __builtin_amdgcn_readfirstlane(e.x & 0xfffffff);
      const int j = __builtin_amdgcn_readfirstlane(e.y);
      if (draws >= max_dec) {
        bad = kFoldSampleRunaway;
        break;
      }
      const double u = rng_uniform(stream, draws++);
      const int d = j - i;
      int win;
      if (type == kSegExt) {
        // Q5[j] = Q5[jl] sc + sum_k Q5[k] Qb(k, jl) au, jl = j - 1 the last base
        const int jl = j - 1;
        const int cj = c[jl];
        win = choose(1 + (jl - 3), [&](int idx) {
          if (idx == 0) return Q5[jl] * scp[1];
          const int k = idx - 1;
          const double v = Qb[D(jl - k, k)];
          return v != 0.0 ? Q5[k] * v * T.au[pair_raw(c[k], cj)] : 0.0;
        }, u, lane);
        if (win < 0) {
          bad = kFoldSampleNoWeight;
        } else if (win == 0) {
          if (jl >= 5) push(kSegExt, 0, jl);
        } else {
          const int k = win - 1;
          add_pair(k, jl);
          if (k >= 5) push(kSegExt, 0, k);
          push(kSegB, k, jl);
        }
      } else if (type == kSegB) {
        const int t = fold_ptype(c, lp, n, ngu, i, j);
        const bool closes = t != 0 && !(ncg && is_gu(t));  // hairpin and multiloop allowed
        const int nint = d >= 6 ? (min(30, d - 6) + 1) * 31 : 0;
        const int nml = closes && d > 10 ? d - 10 : 0;  // e = 5 .. d - 6
        win = t == 0 ? -1 : choose(1 + nint + nml, [&](int idx) {
          if (idx == 0) return closes ? T.hp[d - 1] * T.au[t] * scp[d + 1] : 0.0;
          if (idx <= nint) {
            // (p, q) = (i+1+n1, j-1-n2), n1 + n2 <= 30, q >= p + 4
            const int n1 = (idx - 1) / 31, n2 = (idx - 1) % 31;
            if (n1 + n2 > 30 || n1 + n2 > d - 6) return 0.0;
            const int p = i + 1 + n1;
            const double v = Qb[D(d - 2 - n1 - n2, p)];
            return v != 0.0 ? v * fold_interior(T, t, pair_raw(c[j - 1 - n2], c[p]), n1, n2, ncg) *
                                  scp[n1 + n2 + 2]
                            : 0.0;
          }
          const int el = 5 + (idx - 1 - nint);
          return Qm[D(el - 1, i + 1)] * Qm1[D(d - el - 2, i + el + 1)] * T.mlc * T.au[t] * scp[2];
        }, u, lane);
        if (win < 0) {
          bad = kFoldSampleNoWeight;
        } else if (win == 0) {
          // hairpin
        } else if (win <= nint) {
          const int n1 = (win - 1) / 31, n2 = (win - 1) % 31;
          add_pair(i + 1 + n1, j - 1 - n2);
          push(kSegB, i + 1 + n1, j - 1 - n2);
        } else {
          const int el = 5 + (win - 1 - nint);
          push(kSegM, i + 1, i + el);
          push(kSegM1, i + el + 1, j - 1);
        }
      } else if (type == kSegM) {
        // Qm(i, j) = sum_u (sc^(u-i) + Qm(i, u-1)) Qm1(u, j), u = i .. j - 4
        win = d < 4 ? -1 : choose(2 * (d - 3), [&](int idx) {
          const int uu = i + (idx >> 1);
          const double q1 = Qm1[D(j - uu, uu)];
          if (q1 == 0.0) return 0.0;
          if (idx & 1) return uu - 1 >= i ? Qm[D(uu - 1 - i, i)] * q1 : 0.0;
          return scp[uu - i] * q1;
        }, u, lane);
        if (win < 0) {
          bad = kFoldSampleNoWeight;
        } else {
          const int uu = i + (win >> 1);
          if (win & 1) push(kSegM, i, uu - 1);
          push(kSegM1, uu, j);
        }
      } else {
        // Qm1(i, j) = sum_l Qb(i, l) mli au sc^(j-l), l = i + 4 .. j
        const int ci = c[i];
        win = d < 4 ? -1 : choose(d - 3, [&](int idx) {
          const int l = i + 4 + idx;
          const double v = Qb[D(l - i, i)];
          return v != 0.0 ? v * T.mli * T.au[pair_raw(ci, c[l])] * scp[j - l] : 0.0;
        }, u, lane);
        if (win < 0) {
          bad = kFoldSampleNoWeight;
        } else {
          add_pair(i, i + 4 + win);
          push(kSegB, i, i + 4 + win);
        }
      }
    }
    if (bad) {  // abandon the sample; the host fails the call
      if (lane == 0) *S.status = bad;
    }
  }
}

size_t fold_sample_lds_bytes(const FoldLaunch& P, int max_n) {
  return (size_t)P.n_tab_pad * 8 + (size_t)kSampleWaves * fold_sample_stack_cap(max_n) * sizeof(int2) +
         (size_t)(max_n + 15) / 16 * 16;
}

hipError_t launch_fold_sample(const FoldSampleLaunch& S0, int n_seqs, int max_n, hipStream_t st) {
  if (n_seqs <= 0 || S0.n_samples <= 0) return hipSuccess;
  FoldSampleLaunch S = S0;
  S.F.max_n = max_n;
  const size_t lds = fold_sample_lds_bytes(S.F, max_n);
  if (lds > kFoldLdsMax) return hipErrorInvalidValue;
  // enough workgroups to fill the chip when the call has few sequences
  const int per_wg = (S.n_samples + kSampleWaves - 1) / kSampleWaves;
  int gy = (2048 + n_seqs - 1) / n_seqs;
  gy = gy < 1 ? 1 : (gy > per_wg ? per_wg : gy);
  return launch_fold_kernel(sk_fold_sample_kernel, S, dim3(n_seqs, gy), kSampleWaves * 64, lds, st);
}

}  // namespace sk
