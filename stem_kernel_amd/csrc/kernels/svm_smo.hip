// Batched C-SVC training on CDNA4 (gfx950): libsvm's SMO solver, without
// shrinking or with it (two instantiations of one kernel), one workgroup per
// (training subset, C) problem over one Gram resident in device memory.
//
// Reference: Solver::Solve  libsvm/solver.cpp:81-349, select_working_set
//   :352-451, calculate_rho :554-592, SVC_Q libsvm/qmatrix.cpp:339-362; with
//   shrinking also swap_index :47-57, reconstruct_gradient :61-79,
//   do_shrinking :475-552; the
//   arithmetic contract is the one csrc/host/svm_train.cpp restates (float Q
//   entries and quad_coef, double everything else, no fused multiply-add),
//   and the alphas are that file's bit for bit: every rounded operation below
//   is an explicit __d*_rn / __f*_rn, which the compiler does not contract.
//
// Schedule.  A workgroup of T threads (T = 64, 256 or 1,024: the size
// classes, kSvmElems elements per thread each, so n_train <= 256, 1,024 or
// 4,096) solves one problem.  Thread tid owns the training examples
// k = tid, tid + T, ...: their G and alpha (double), QD (float), label, Gram
// index and bound status stay in registers for the whole solve, and a row of
// the Gram is gathered with consecutive lanes on consecutive k.  One iteration:
//   1. every thread scans its elements for the maximiser of -y G over I_up;
//      a butterfly over the wave, then over the waves through LDS, combines
//      (value, index) pairs -- larger value, of equal values the larger index,
//      which is what a sequential scan with >= keeps.  The thread that owns
//      the wave's winner writes the wave's record with that element's alpha
//      and QD, so after one barrier every thread knows i, G_i, alpha_i, QD_i.
//   2. every thread reads its entries of row t_i, computes obj_diff for its
//      elements of I_low and Gmax2; the same combine with (smaller value,
//      larger index); the winner's owner adds G_j, alpha_j, QD_j.  Second
//      barrier.
//   3. the stopping test, then the two-variable update: computed by every
//      thread from the same values (uniform, so no broadcast and no third
//      barrier); the owners of i and j keep the new alphas and statuses.
//   4. every thread reads its entries of row t_j and updates its G.
// Two barriers and two dependent row gathers per iteration.  The Gram is read
// by row only (row t_i for Q_i), as the reference's kernel_precomputed does.
//
// After the solve: rho's sum over the free variables and obj's sum are added
// up in index order by one thread from LDS (so rho and obj are the host
// path's bits too; 2 x n_train dependent adds, microseconds); the bounds,
// n_free and n_bound by exact reductions.  Decision values of the test list:
// one wave per test example, lanes over the training examples, a butterfly
// sum -- the one place where the order of a sum differs from the host's.
//
// Shrinking (SHRINK = true; csrc/host/svm_train.cpp: ShrinkSmo is the same
// restated on the host).  "Element k" above becomes "position k" of the
// reference's permuted problem: a thread's registers hold whatever example
// occupies its positions, with that example's training index (aset) and
// G_bar next to G.  Steps 1, 2 and 4 run over the positions < active.  When
// alpha_i or alpha_j enters or leaves its upper bound (known to every thread:
// the status is a function of alpha), every thread adds -+ C Q[k] to its
// G_bar over all l positions, reading the row's entries of its inactive
// positions too.  Every min(l, 1000) iterations a shrink event: Gmax1 and
// Gmax2 by exact max reductions; every thread writes be_shrunken of its
// positions as a byte to LDS; thread 0 runs the reference's two-pointer loop
// on the bytes, swapping them as the reference swaps state and recording the
// swaps in a permutation; then every thread gathers its state through that
// permutation, one array at a time through LDS (nothing to gather when no
// swap was made, the common case).  The serial part is O(l) LDS operations
// per event and stays serial.  reconstruct_gradient: the free active alphas
// go to LDS by position (-1 elsewhere), every thread walks the positions in
// ascending order -- a uniform loop -- and adds alpha_i Q_i[j] to the G of
// its inactive positions, so every G[j] receives its terms in the
// reference's order with two roundings each.  The unshrink branch is
// reconstruct, fresh bytes, the mirror loop from the tail and the gather
// again.  The epilogue's sequential sums run over positions, which is the
// reference's order; alphas are written to their training indices.
//
// LDS per workgroup: 12 bytes per element slot (48 KiB in the largest class)
// and the waves' records; the shrink event reuses the slots.  No atomics, no
// inline assembly.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../host/runtime.h"
#include "../host/svm_train.h"

namespace sk {

namespace {

struct SvmProb {
  int64_t max_iter;
  double Cp, Cn, eps;
  int32_t train_off, n_train, test_off, n_test;
};
struct SvmLaunch {
  const double* gram;
  int32_t n;
  const signed char* ypos;  // per example of the Gram: 1 when its label is > 0
  const int32_t* train;     // the problems' training lists, concatenated
  const int32_t* test;
  const SvmProb* prob;
  const int32_t* which;     // the problems of this launch's class
  double* alpha;
  double* dec;
  sk_svm_solution* sol;
  sk_svm_shrink_info* info;  // written by the shrinking solver only
};

struct RecI {  // a wave's candidate for i
  double v, alpha;
  float qd;
  int32_t idx;
};
struct RecJ {  // a wave's candidate for j
  double od, g, alpha;
  float qd;
  int32_t idx;
};

constexpr double kSvmTau = 1e-12;
enum : int { kStLower = 0, kStUpper = 1, kStFree = 2, kStAbsent = 3 };

__device__ __forceinline__ double shfl_xor_f64(double v, int m) { return __shfl_xor(v, m, 64); }

// SHRINK: libsvm's shrinking (Solve(..., shrinking = 1)); its additions are
// described above ("Shrinking") and compiled into that instantiation only.
template <int T, bool SHRINK>
__global__ void __launch_bounds__(T) sk_svm_smo_kernel(SvmLaunch L) {
  constexpr int E = kSvmElems, W = T / 64, CAP = T * E;
  __shared__ double s_val[CAP];
  __shared__ int32_t s_ty[CAP];  // (Gram index << 1) | (y > 0)
  __shared__ RecI s_ri[W];
  __shared__ RecJ s_rj[W];
  __shared__ double s_g2[W];
  __shared__ double s_ub[W], s_lb[W];
  __shared__ int32_t s_nf[W], s_nb[W];
  __shared__ double s_seq[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SvmProb P = L.prob[L.which[blockIdx.x]];
  const int l = P.n_train;
  const size_t n = (size_t)L.n;
  const double* __restrict__ K = L.gram;
  const int32_t* __restrict__ tr = L.train + P.train_off;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);

  int tk[E], yk[E], st[E];
  float qd[E], qi[E], qj[E];
  double G[E], al[E];
  // SHRINK: position k = e * T + tid holds training example aset[e]; Gb is G_bar
  int aset[E];
  double Gb[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int k = e * T + tid;
    tk[e] = 0, yk[e] = 1, st[e] = kStAbsent, qd[e] = 0.f, qi[e] = 0.f, qj[e] = 0.f, G[e] = 0.0, al[e] = 0.0;
    aset[e] = k, Gb[e] = 0.0;
    if (k < l) {
      const int t = tr[k];
      tk[e] = t;
      yk[e] = L.ypos[t] ? 1 : -1;
      st[e] = kStLower;
      qd[e] = (float)K[(size_t)t * n + t];
      G[e] = -1.0;
      s_ty[k] = (t << 1) | (yk[e] > 0 ? 1 : 0);
    }
  }
  __syncthreads();

  int64_t iter = 0;
  int status = SK_SVM_CONVERGED;
  // SHRINK: the positions < active are selected from and updated
  int active = l;
  auto live = [&](int e) {
    if constexpr (SHRINK) return e * T + tid < active;
    else return st[e] != kStAbsent;
  };
  sk_svm_shrink_info info = {0, 0, l, 0, 0, 0, 0};

  // s_val[k] = X[position k]; X[e] = s_val[sp[e]]: the state moves to its new positions
  auto gather = [&](double(&X)[E], const int(&sp)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (st[e] != kStAbsent) s_val[e * T + tid] = X[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (st[e] != kStAbsent) X[e] = s_val[sp[e]];
    __syncthreads();
  };
  // be_shrunken of every position as a byte in s_val's first CAP bytes, and
  // the identity permutation as 16-bit entries in the 2 CAP bytes after them
  static_assert(CAP <= 65536 && CAP % 2 == 0, "positions are 16-bit entries of s_val");
  unsigned char* const s_flag = reinterpret_cast<unsigned char*>(s_val);
  unsigned short* const s_src = reinterpret_cast<unsigned short*>(s_val) + CAP / 2;
  auto write_flags = [&](double g1, double g2) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (st[e] == kStAbsent) continue;
      bool f = false;
      if (st[e] == kStUpper) f = yk[e] > 0 ? -G[e] > g1 : -G[e] > g2;
      else if (st[e] == kStLower) f = yk[e] > 0 ? G[e] > g2 : G[e] > g1;
      s_flag[e * T + tid] = f ? 1 : 0;
      s_src[e * T + tid] = (unsigned short)(e * T + tid);
    }
    __syncthreads();
  };
  // after thread 0's serial loop (new active size in s_nf[0], "a swap was
  // made" in s_nb[0], the permutation in s_src): every array of the state,
  // one at a time through s_val; status, QD and aset as one 64-bit word
  auto apply_permutation = [&]() {
    __syncthreads();
    active = s_nf[0];
    if (!s_nb[0]) return;  // uniform
    int sp[E];
#pragma unroll
    for (int e = 0; e < E; ++e) sp[e] = st[e] != kStAbsent ? (int)s_src[e * T + tid] : 0;
    __syncthreads();
    gather(G, sp);
    gather(Gb, sp);
    gather(al, sp);
    double w[E];
#pragma unroll
    for (int e = 0; e < E; ++e)
      w[e] = __longlong_as_double(((long long)((aset[e] << 2) | st[e]) << 32) | (long long)__float_as_uint(qd[e]));
    gather(w, sp);
    int ty[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (st[e] == kStAbsent) continue;
      const long long b = __double_as_longlong(w[e]);
      qd[e] = __uint_as_float((unsigned)(b & 0xffffffffll));
      st[e] = (int)(b >> 32) & 3;
      aset[e] = (int)(b >> 34);
      ty[e] = s_ty[sp[e]];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (st[e] != kStAbsent) s_ty[e * T + tid] = ty[e], tk[e] = ty[e] >> 1, yk[e] = (ty[e] & 1) ? 1 : -1;
    __syncthreads();
  };
  // reconstruct_gradient: G of the positions in [active, l) from G_bar + p
  // and the free active positions i in ascending order (their alphas by
  // position in s_val, -1 for the others: the loop over i is uniform), lanes
  // on consecutive positions of row t_i, two roundings per term
  auto reconstruct = [&]() {
    if (active == l) return;  // uniform
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (st[e] == kStAbsent) continue;
      const int k = e * T + tid;
      s_val[k] = (k < active && st[e] == kStFree) ? al[e] : -1.0;
      if (k >= active) G[e] = __dadd_rn(Gb[e], -1.0);
    }
    __syncthreads();
    for (int i = 0; i < active; ++i) {
      const double a = s_val[i];
      if (a < 0) continue;
      const int ty = s_ty[i];
      const int y_i = (ty & 1) ? 1 : -1;
      const double* __restrict__ ri = K + (size_t)(ty >> 1) * n;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (st[e] != kStAbsent && e * T + tid >= active) {
          const float q = (float)((double)(y_i * yk[e]) * ri[tk[e]]);
          G[e] = __dadd_rn(G[e], __dmul_rn(a, (double)q));
        }
    }
    __syncthreads();
  };
  // do_shrinking
  bool unshrunk = false;
  auto shrink_event = [&]() {
    ++info.shrink_calls;
    const int before = active;
    double g1 = -inf, g2 = -inf;  // max of -y G over I_up, of y G over I_low
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (!live(e)) continue;
      if (yk[e] > 0) {
        if (st[e] != kStUpper && -G[e] >= g1) g1 = -G[e];
        if (st[e] != kStLower && G[e] >= g2) g2 = G[e];
      } else {
        if (st[e] != kStUpper && -G[e] >= g2) g2 = -G[e];
        if (st[e] != kStLower && G[e] >= g1) g1 = G[e];
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double o1 = shfl_xor_f64(g1, m), o2 = shfl_xor_f64(g2, m);
      g1 = o1 > g1 ? o1 : g1;
      g2 = o2 > g2 ? o2 : g2;
    }
    if (lane == 0) s_ub[wave] = g1, s_lb[wave] = g2;
    __syncthreads();
    g1 = -inf, g2 = -inf;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      g1 = s_ub[w] > g1 ? s_ub[w] : g1;
      g2 = s_lb[w] > g2 ? s_lb[w] : g2;
    }
    write_flags(g1, g2);
    if (tid == 0) {  // the two-pointer loop from both ends
      int a = active, moved = 0;
      for (int k = 0; k < a; ++k)
        if (s_flag[k])
          for (--a; a > k; --a)
            if (!s_flag[a]) {
              s_flag[k] = 0, s_flag[a] = 1;
              const unsigned short x = s_src[k];
              s_src[k] = s_src[a], s_src[a] = x;
              moved = 1;
              break;
            }
      s_nf[0] = a, s_nb[0] = moved;
    }
    apply_permutation();
    if (!unshrunk && !(__dadd_rn(g1, g2) > __dmul_rn(P.eps, 10.0))) {
      unshrunk = true;
      info.unshrunk = 1;
      reconstruct();
      write_flags(g1, g2);
      if (tid == 0) {  // the mirror loop from the tail
        int a = active, moved = 0;
        for (int k = l - 1; k >= a; --k)
          if (!s_flag[k]) {
            for (; a < k; ++a)
              if (s_flag[a]) {
                s_flag[k] = 1, s_flag[a] = 0;
                const unsigned short x = s_src[k];
                s_src[k] = s_src[a], s_src[a] = x;
                moved = 1;
                break;
              }
            ++a;
          }
        s_nf[0] = a, s_nb[0] = moved;
      }
      apply_permutation();
      if (active > before) info.regrown = 1;
    }
    if (active < before) ++info.shrunk_calls;
    info.min_active = active < info.min_active ? active : info.min_active;
  };
  const int period = l < 1000 ? l : 1000;
  int counter = period + 1;
  bool again = false, stopped = false, pending = false;

  for (;;) {
    if constexpr (SHRINK) {
      if (!again && --counter == 0) {
        counter = period;
        shrink_event();
      }
    }
    // ---- 1. i: the last maximiser of -y G over I_up
    double v = -inf;
    int idx = -1;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (!live(e)) continue;
      const int k = e * T + tid;
      if (yk[e] > 0) {
        if (st[e] != kStUpper && -G[e] >= v) v = -G[e], idx = k;
      } else {
        if (st[e] != kStLower && G[e] >= v) v = G[e], idx = k;
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double ov = shfl_xor_f64(v, m);
      const int oi = __shfl_xor(idx, m, 64);
      if (ov > v || (ov == v && oi > idx)) v = ov, idx = oi;
    }
    if (idx >= 0 ? (idx & (T - 1)) == tid : lane == 0) {
      const int slot = idx >= 0 ? idx / T : 0;
      RecI r;
      r.v = v, r.idx = idx, r.alpha = 0.0, r.qd = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (e == slot) r.alpha = al[e], r.qd = qd[e];
      s_ri[wave] = r;
    }
    __syncthreads();
    double gmax = -inf, ai0 = 0.0;
    float qd_i = 0.f;
    int i = -1;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const RecI r = s_ri[w];
      if (r.v > gmax || (r.v == gmax && r.idx > i)) gmax = r.v, i = r.idx, ai0 = r.alpha, qd_i = r.qd;
    }
    int y_i = 1;
    const double* __restrict__ ri = K;
    if (i >= 0) {
      const int ty = s_ty[i];
      y_i = (ty & 1) ? 1 : -1;
      ri = K + (size_t)(ty >> 1) * n;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (live(e)) qi[e] = (float)((double)(y_i * yk[e]) * ri[tk[e]]);
    }

    // ---- 2. j: the last minimiser of the objective's decrease over I_low
    double od = inf, g2 = -inf;
    int jdx = -1;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (!live(e)) continue;
      double gd;
      float qf;
      if (yk[e] > 0) {
        if (st[e] == kStLower) continue;
        gd = __dadd_rn(gmax, G[e]);
        if (G[e] >= g2) g2 = G[e];
        if (!(gd > 0)) continue;
        qf = __fsub_rn(__fadd_rn(qd_i, qd[e]), __fmul_rn((float)(2 * y_i), qi[e]));
      } else {
        if (st[e] == kStUpper) continue;
        gd = __dsub_rn(gmax, G[e]);
        if (-G[e] >= g2) g2 = -G[e];
        if (!(gd > 0)) continue;
        qf = __fadd_rn(__fadd_rn(qd_i, qd[e]), __fmul_rn((float)(2 * y_i), qi[e]));
      }
      const double qc = (double)qf;
      const double od_e = -__ddiv_rn(__dmul_rn(gd, gd), qc > 0 ? qc : kSvmTau);
      if (od_e <= od) od = od_e, jdx = e * T + tid;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double oo = shfl_xor_f64(od, m);
      const int oj = __shfl_xor(jdx, m, 64);
      const double og = shfl_xor_f64(g2, m);
      if (oo < od || (oo == od && oj > jdx)) od = oo, jdx = oj;
      if (og > g2) g2 = og;
    }
    if (jdx >= 0 ? (jdx & (T - 1)) == tid : lane == 0) {
      const int slot = jdx >= 0 ? jdx / T : 0;
      RecJ r;
      r.od = od, r.idx = jdx, r.g = 0.0, r.alpha = 0.0, r.qd = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (e == slot) r.g = G[e], r.alpha = al[e], r.qd = qd[e];
      s_rj[wave] = r;
    }
    if (lane == 0) s_g2[wave] = g2;
    __syncthreads();
    double od_min = inf, gmax2 = -inf, G_j = 0.0, aj0 = 0.0;
    float qd_j = 0.f;
    int j = -1;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const RecJ r = s_rj[w];
      if (r.od < od_min || (r.od == od_min && r.idx > j))
        od_min = r.od, j = r.idx, G_j = r.g, aj0 = r.alpha, qd_j = r.qd;
      const double g = s_g2[w];
      if (g > gmax2) gmax2 = g;
    }

    // ---- 3. stop, or update alpha_i and alpha_j (every thread, same values)
    if constexpr (!SHRINK) {
      if (__dadd_rn(gmax, gmax2) < P.eps) break;
      if (i < 0 || j < 0) {
        status = SK_SVM_NO_PAIR;
        break;
      }
      if (iter == P.max_iter) {
        status = SK_SVM_NOT_CONVERGED;
        break;
      }
    } else {
      // An optimal selection on a shrunk set is not the end: reconstruct the
      // gradient, restore the whole set and select again (`again`); a pair
      // found then resumes the loop, with a shrink at the next iteration.
      // max_iter (and a missing pair) end the solve the same way: as if the
      // selection had reported optimal, twice.
      bool found = false;
      const bool after_reconstruction = pending;
      pending = false;
      if (__dadd_rn(gmax, gmax2) < P.eps) {
        if (active < l) ++info.reconstructions, pending = true;
      } else if (i < 0 || j < 0) {
        status = SK_SVM_NO_PAIR, stopped = true;
      } else if (iter == P.max_iter) {
        status = SK_SVM_NOT_CONVERGED, stopped = true;
      } else {
        if (after_reconstruction) ++info.resumed;
        found = true;
      }
      if (!found) {
        if (again) break;
        reconstruct();
        active = l;
        if (stopped) break;
        again = true;
        continue;
      }
      if (again) counter = 1, again = false;
    }
    ++iter;
    const int tyj = s_ty[j];
    const int y_j = (tyj & 1) ? 1 : -1;
    const double* __restrict__ rj = K + (size_t)(tyj >> 1) * n;
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (live(e)) qj[e] = (float)((double)(y_j * yk[e]) * rj[tk[e]]);
    const float q_ij = (float)((double)(y_i * y_j) * ri[tyj >> 1]);
    const double G_i = y_i > 0 ? -gmax : gmax;
    const double Ci = y_i > 0 ? P.Cp : P.Cn, Cj = y_j > 0 ? P.Cp : P.Cn;
    double ai = ai0, aj = aj0;
    if (y_i != y_j) {
      const float qf = __fadd_rn(__fadd_rn(qd_i, qd_j), __fmul_rn(2.f, q_ij));
      double qc = (double)qf;
      if (qc <= 0) qc = kSvmTau;
      const double delta = __ddiv_rn(__dsub_rn(-G_i, G_j), qc);
      const double diff = __dsub_rn(ai, aj);
      ai = __dadd_rn(ai, delta);
      aj = __dadd_rn(aj, delta);
      if (diff > 0) {
        if (aj < 0) aj = 0, ai = diff;
      } else {
        if (ai < 0) ai = 0, aj = -diff;
      }
      if (diff > __dsub_rn(Ci, Cj)) {
        if (ai > Ci) ai = Ci, aj = __dsub_rn(Ci, diff);
      } else {
        if (aj > Cj) aj = Cj, ai = __dadd_rn(Cj, diff);
      }
    } else {
      const float qf = __fsub_rn(__fadd_rn(qd_i, qd_j), __fmul_rn(2.f, q_ij));
      double qc = (double)qf;
      if (qc <= 0) qc = kSvmTau;
      const double delta = __ddiv_rn(__dsub_rn(G_i, G_j), qc);
      const double sum = __dadd_rn(ai, aj);
      ai = __dsub_rn(ai, delta);
      aj = __dadd_rn(aj, delta);
      if (sum > Ci) {
        if (ai > Ci) ai = Ci, aj = __dsub_rn(sum, Ci);
      } else {
        if (aj < 0) aj = 0, ai = sum;
      }
      if (sum > Cj) {
        if (aj > Cj) aj = Cj, ai = __dsub_rn(sum, Cj);
      } else {
        if (ai < 0) ai = 0, aj = sum;
      }
    }
    const double dai = __dsub_rn(ai, ai0), daj = __dsub_rn(aj, aj0);

    // ---- 4. G, and the owners' alphas
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (live(e))
        G[e] = __dadd_rn(G[e], __dadd_rn(__dmul_rn((double)qi[e], dai), __dmul_rn((double)qj[e], daj)));
    if constexpr (SHRINK) {
      // G_bar: -+ C Q[k] over all l positions when i, then j, leaves or
      // enters its upper bound (the status is a function of alpha: uniform)
      if ((ai0 >= Ci) != (ai >= Ci)) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (st[e] == kStAbsent) continue;
          const float q = live(e) ? qi[e] : (float)((double)(y_i * yk[e]) * ri[tk[e]]);
          const double cq = __dmul_rn(Ci, (double)q);
          Gb[e] = ai0 >= Ci ? __dsub_rn(Gb[e], cq) : __dadd_rn(Gb[e], cq);
        }
      }
      if ((aj0 >= Cj) != (aj >= Cj)) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (st[e] == kStAbsent) continue;
          const float q = live(e) ? qj[e] : (float)((double)(y_j * yk[e]) * rj[tk[e]]);
          const double cq = __dmul_rn(Cj, (double)q);
          Gb[e] = aj0 >= Cj ? __dsub_rn(Gb[e], cq) : __dadd_rn(Gb[e], cq);
        }
      }
    }
    if ((i & (T - 1)) == tid) {
      const int slot = i / T;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (e == slot) al[e] = ai, st[e] = ai >= Ci ? kStUpper : ai <= 0 ? kStLower : kStFree;
    }
    if ((j & (T - 1)) == tid) {
      const int slot = j / T;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (e == slot) al[e] = aj, st[e] = aj >= Cj ? kStUpper : aj <= 0 ? kStLower : kStFree;
    }
  }

  // ---- rho: the free variables' y G summed in index order (adding +0.0 for
  // the others changes no bit: the sum starts at +0.0); bounds by reduction
  double ub = inf, lb = -inf;
  int nf = 0, nb = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    if (st[e] == kStAbsent) continue;
    const double yg = yk[e] > 0 ? G[e] : -G[e];
    double f = 0.0;
    if (st[e] == kStUpper) {
      ++nb;
      if (yk[e] < 0) ub = yg < ub ? yg : ub;
      else lb = yg > lb ? yg : lb;
    } else if (st[e] == kStLower) {
      if (yk[e] > 0) ub = yg < ub ? yg : ub;
      else lb = yg > lb ? yg : lb;
    } else {
      ++nf;
      f = yg;
    }
    s_val[e * T + tid] = f;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double ou = shfl_xor_f64(ub, m), ol = shfl_xor_f64(lb, m);
    ub = ou < ub ? ou : ub;
    lb = ol > lb ? ol : lb;
    nf += __shfl_xor(nf, m, 64);
    nb += __shfl_xor(nb, m, 64);
  }
  if (lane == 0) s_ub[wave] = ub, s_lb[wave] = lb, s_nf[wave] = nf, s_nb[wave] = nb;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int k = 0; k < l; ++k) sum = __dadd_rn(sum, s_val[k]);
    s_seq[0] = sum;
  }
  ub = inf, lb = -inf, nf = 0, nb = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    ub = s_ub[w] < ub ? s_ub[w] : ub;
    lb = s_lb[w] > lb ? s_lb[w] : lb;
    nf += s_nf[w];
    nb += s_nb[w];
  }
  __syncthreads();
  const double rho = nf > 0 ? __ddiv_rn(s_seq[0], (double)nf) : __ddiv_rn(__dadd_rn(ub, lb), 2.0);
  // ---- obj = sum alpha (G + p) / 2, in index order
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (st[e] != kStAbsent) s_val[e * T + tid] = __dmul_rn(al[e], __dadd_rn(G[e], -1.0));
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int k = 0; k < l; ++k) sum = __dadd_rn(sum, s_val[k]);
    sk_svm_solution S;
    S.rho = rho;
    S.obj = __ddiv_rn(sum, 2.0);
    S.iterations = iter;
    S.status = status;
    S.n_free = nf;
    S.n_bound = nb;
    L.sol[L.which[blockIdx.x]] = S;
    if constexpr (SHRINK) L.info[L.which[blockIdx.x]] = info;
  }
  __syncthreads();
  // ---- alphas out; decision values of the test list
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (st[e] != kStAbsent) {
      const int k = e * T + tid;
      L.alpha[P.train_off + (SHRINK ? aset[e] : k)] = al[e];
      s_val[k] = yk[e] > 0 ? al[e] : -al[e];
    }
  __syncthreads();
  for (int q = wave; q < P.n_test; q += W) {
    const double* __restrict__ rs = K + (size_t)L.test[P.test_off + q] * n;
    double sum = 0.0;
    for (int a = lane; a < l; a += 64) {
      const double c = s_val[a];
      if (c != 0.0) sum = __dadd_rn(sum, __dmul_rn(c, rs[s_ty[a] >> 1]));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum = __dadd_rn(sum, shfl_xor_f64(sum, m));
    if (lane == 0) L.dec[P.test_off + q] = __dsub_rn(sum, rho);
  }
}

template <int T>
hipError_t launch_class(const SvmLaunch& L, bool shrinking, int grid, hipStream_t st) {
  if (shrinking) hipLaunchKernelGGL((sk_svm_smo_kernel<T, true>), dim3(grid), dim3(T), 0, st, L);
  else hipLaunchKernelGGL((sk_svm_smo_kernel<T, false>), dim3(grid), dim3(T), 0, st, L);
  return hipGetLastError();
}

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

}  // namespace
}  // namespace sk

#define SK_SVM_HIP(expr)                                                                                 \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess)                                                                                \
      return sk::ctx_fail(ctx, SK_ERR_HIP, std::string("sk_svm_train_batch: " #expr ": ") + hipGetErrorString(_e)); \
  } while (0)

extern "C" int sk_svm_train_batch_ex(sk_context* ctx, const double* gram, int32_t n, const double* labels,
                                     const sk_svm_problem* problems, int32_t n_problems, int32_t shrinking,
                                     double* alpha_out, double* dec_out, sk_svm_solution* solutions,
                                     sk_svm_shrink_info* info) {
  if (!ctx) return SK_ERR_INVALID;
  try {
    sk::lev_reset(ctx);
    std::string err;
    int64_t sum_train = 0, sum_test = 0;
    const int rc = sk::svm_check_batch(gram, n, labels, problems, n_problems, alpha_out, dec_out, solutions,
                                       sk::kSvmMaxTrain, &sum_train, &sum_test, err);
    if (rc) return sk::ctx_fail(ctx, rc, err);
    if (n_problems == 0) return SK_OK;
    if (sum_train > INT32_MAX || sum_test > INT32_MAX)
      return sk::ctx_fail(ctx, SK_ERR_UNSUPPORTED, "sk_svm_train_batch: over 2^31 list entries in one call");

    // host images: labels' signs, the lists concatenated, the descriptors, the classes' problems
    std::vector<signed char> ypos(n);
    for (int32_t k = 0; k < n; ++k) ypos[k] = labels[k] > 0 ? 1 : 0;
    std::vector<int32_t> train((size_t)sum_train), test((size_t)sum_test);
    std::vector<sk::SvmProb> prob(n_problems);
    std::vector<int32_t> which[sk::kSvmClasses];
    int32_t to = 0, so = 0;
    for (int p = 0; p < n_problems; ++p) {
      const sk_svm_problem& P = problems[p];
      sk::SvmProb& D = prob[p];
      D.max_iter = P.max_iter;
      D.Cp = P.Cp, D.Cn = P.Cn, D.eps = P.eps;
      D.train_off = to, D.n_train = P.n_train, D.test_off = so, D.n_test = P.n_test;
      std::memcpy(train.data() + to, P.train, (size_t)P.n_train * 4);
      if (P.n_test) std::memcpy(test.data() + so, P.test, (size_t)P.n_test * 4);
      to += P.n_train;
      so += P.n_test;
      int c = 0;
      while (P.n_train > sk::kSvmThreads[c] * sk::kSvmElems) ++c;
      which[c].push_back(p);
    }
    std::vector<int32_t> which_all;
    int32_t which_off[sk::kSvmClasses];
    for (int c = 0; c < sk::kSvmClasses; ++c) {
      which_off[c] = (int32_t)which_all.size();
      which_all.insert(which_all.end(), which[c].begin(), which[c].end());
    }

    SK_SVM_HIP(hipSetDevice(sk::ctx_device(ctx)));
    // a fresh timing set for the launch events below, collected before this
    // call returns (lev_collect), so no call_finish: the call is synchronous and
    // stages nothing.  On an asynchronous context call_begin also advances the
    // staging ring by one slot, which this call leaves empty (sk_bpla_gradients
    // does the same).
    SK_SVM_HIP(sk::call_begin(ctx));
    hipStream_t S = sk::ctx_stream(ctx);
    // one device arena
    size_t off = 0;
    auto take = [&](size_t bytes) {
      const size_t at = off;
      off += (bytes + 255) & ~(size_t)255;
      return at;
    };
    const size_t o_gram = take((size_t)n * n * 8), o_y = take((size_t)n), o_tr = take((size_t)sum_train * 4),
                 o_ts = take((size_t)sum_test * 4), o_pr = take((size_t)n_problems * sizeof(sk::SvmProb)),
                 o_wh = take((size_t)n_problems * 4), o_al = take((size_t)sum_train * 8),
                 o_de = take((size_t)sum_test * 8), o_so = take((size_t)n_problems * sizeof(sk_svm_solution)),
                 o_in = take((size_t)n_problems * sizeof(sk_svm_shrink_info));
    sk::DevBuf buf;
    if (hipMalloc(&buf.p, off) != hipSuccess) {
      (void)hipGetLastError();
      return sk::ctx_fail(ctx, SK_ERR_ALLOC, "sk_svm_train_batch: device memory for the Gram and the lists");
    }
    char* base = static_cast<char*>(buf.p);
    auto up = [&](size_t at, const void* src, size_t bytes) {
      return bytes ? hipMemcpyAsync(base + at, src, bytes, hipMemcpyHostToDevice, S) : hipSuccess;
    };
    SK_SVM_HIP(up(o_gram, gram, (size_t)n * n * 8));
    SK_SVM_HIP(up(o_y, ypos.data(), (size_t)n));
    SK_SVM_HIP(up(o_tr, train.data(), (size_t)sum_train * 4));
    SK_SVM_HIP(up(o_ts, test.data(), (size_t)sum_test * 4));
    SK_SVM_HIP(up(o_pr, prob.data(), (size_t)n_problems * sizeof(sk::SvmProb)));
    SK_SVM_HIP(up(o_wh, which_all.data(), (size_t)n_problems * 4));
    sk::SvmLaunch L;
    L.gram = reinterpret_cast<const double*>(base + o_gram);
    L.n = n;
    L.ypos = reinterpret_cast<const signed char*>(base + o_y);
    L.train = reinterpret_cast<const int32_t*>(base + o_tr);
    L.test = reinterpret_cast<const int32_t*>(base + o_ts);
    L.prob = reinterpret_cast<const sk::SvmProb*>(base + o_pr);
    L.alpha = reinterpret_cast<double*>(base + o_al);
    L.dec = reinterpret_cast<double*>(base + o_de);
    L.sol = reinterpret_cast<sk_svm_solution*>(base + o_so);
    L.info = reinterpret_cast<sk_svm_shrink_info*>(base + o_in);
    // largest class first: its workgroups run longest
    for (int c = sk::kSvmClasses - 1; c >= 0; --c) {
      if (which[c].empty()) continue;
      L.which = reinterpret_cast<const int32_t*>(base + o_wh) + which_off[c];
      const int grid = (int)which[c].size();
      SK_SVM_HIP(sk::lev_mark(ctx, S));
      if (c == 0) SK_SVM_HIP(sk::launch_class<sk::kSvmThreads[0]>(L, shrinking != 0, grid, S));
      if (c == 1) SK_SVM_HIP(sk::launch_class<sk::kSvmThreads[1]>(L, shrinking != 0, grid, S));
      if (c == 2) SK_SVM_HIP(sk::launch_class<sk::kSvmThreads[2]>(L, shrinking != 0, grid, S));
      SK_SVM_HIP(sk::lev_mark(ctx, S));
    }
    SK_SVM_HIP(hipMemcpyAsync(alpha_out, base + o_al, (size_t)sum_train * 8, hipMemcpyDeviceToHost, S));
    if (sum_test)
      SK_SVM_HIP(hipMemcpyAsync(dec_out, base + o_de, (size_t)sum_test * 8, hipMemcpyDeviceToHost, S));
    SK_SVM_HIP(hipMemcpyAsync(solutions, base + o_so, (size_t)n_problems * sizeof(sk_svm_solution),
                              hipMemcpyDeviceToHost, S));
    if (info && shrinking)
      SK_SVM_HIP(hipMemcpyAsync(info, base + o_in, (size_t)n_problems * sizeof(sk_svm_shrink_info),
                                hipMemcpyDeviceToHost, S));
    SK_SVM_HIP(hipStreamSynchronize(S));
    SK_SVM_HIP(sk::lev_collect(ctx));
    if (info && !shrinking)
      for (int p = 0; p < n_problems; ++p) info[p] = sk_svm_shrink_info{0, 0, problems[p].n_train, 0, 0, 0, 0};
    return SK_OK;
  } catch (const std::bad_alloc&) {
    return sk::ctx_fail(ctx, SK_ERR_ALLOC, "sk_svm_train_batch: host memory");
  }
}

extern "C" int sk_svm_train_batch(sk_context* ctx, const double* gram, int32_t n, const double* labels,
                                  const sk_svm_problem* problems, int32_t n_problems, double* alpha_out,
                                  double* dec_out, sk_svm_solution* solutions) {
  return sk_svm_train_batch_ex(ctx, gram, n, labels, problems, n_problems, 0, alpha_out, dec_out, solutions,
                               nullptr);
}
