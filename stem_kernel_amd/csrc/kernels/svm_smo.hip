// Batched SVM training on CDNA4 (gfx950): libsvm's SMO solver, one workgroup
// per problem over one Gram resident in device memory.  C-SVC without
// shrinking or with it, and without shrinking nu-SVC, one-class, epsilon-SVR
// and nu-SVR ("The general solvers" below): instantiations of one kernel.
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
// Shrinking (SHRINK = true; csrc/host/svm_train.cpp: its Solver is the same
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
// The general solvers (FORM = kFormGeneral, kFormNu; sk_svm_solve_batch): the
// other four formulations of svm_train_one (libsvm/svm.cpp:245-300), without
// shrinking.  The host builds each task's positions as the reference's
// solve_* functions do (svm.cpp:73-234; sk::svm_task_positions): per position
// (Gram index, y), the linear term p and the starting alpha, 2 l positions
// over l examples for the SVR types (SVR_Q, libsvm/qmatrix.cpp:423-475);
// over positions Q_i[k] = y_i y_k (float)K[t_i][t_k] for all three Q classes
// (qmatrix.cpp:339-475).  Size classes go by positions.  What they add:
//   - the initial gradient (solver.cpp:113-135): G = p, then the starting
//     alphas go to LDS by position (-1 at the lower bound) and every thread
//     walks the positions in ascending order -- a uniform loop -- adding
//     alpha_i Q_i[k] to its own positions with two roundings: reconstruct's
//     schedule;
//   - kFormGeneral (one-class, epsilon-SVR): the iteration above, one bound C;
//   - kFormNu (nu-SVC, nu-SVR; Solver_NU::select_working_set
//     solver.cpp:595-705).  Step 1 is two arg-max reductions, over the y = +1
//     and the y = -1 positions, sharing one butterfly and one barrier with two
//     records per wave.  Step 2 needs Q_ip[k] at the y = +1 positions only
//     and Q_in[k] at the y = -1 positions only, so every position gathers one
//     entry, from its own class's row (a class whose index is -1 is skipped);
//     one arg-min over both classes with Gmaxp2 and Gmaxn2 riding along.
//     Once j is known, i is the maximiser of j's class, row i is already in
//     registers at that class's positions and is gathered at the other
//     class's together with row j: at most two entries per position and two
//     dependent gathers per iteration, two barriers.  The pair shares a
//     class, so only the equal-label update is compiled.  What the selection
//     hands to every thread is held in scalar registers (readfirstlane of
//     wave-uniform values), and the loops over the waves' records are
//     unrolled by 8 at most: with that the largest class stays under its 128
//     vector registers without scratch.  No j (the reference would read
//     y[-1]): SK_SVM_NO_PAIR;
//   - the epilogue: calculate_rho (:554-592) or Solver_NU's two-sided one
//     (:799-848, which also gives r) with the per-class sums added by one
//     thread from LDS in position order, obj with the general p, then what
//     svm_train_one keeps: coef = alpha (y / r) with rho / r and obj / (r r)
//     for nu-SVC, alpha for one-class, alpha_k - alpha_{k+l} through LDS for
//     the SVR types; the decision values from coef as above.
// coef, rho, obj, r, the iteration count and the counts are the host path's
// bits (csrc/host/svm_train.cpp: the same Solver).
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
  int32_t pos_off, n_pos, svm_type;  // the general solvers: the task's positions; sk_svm_type
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
  // the general solvers (FORM != kFormCSvc): per position (Gram index << 1) |
  // (y > 0), the linear term and the starting alpha, the tasks' concatenated
  const int32_t* pos_ty;
  const double* pos_p;
  const double* pos_a0;
  sk_svm_task_solution* tsol;
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

// FORM, the formulation a kernel instantiation solves:
//   kFormCSvc     solve_c_svc: p = -1, alpha = 0, bounds Cp / Cn (the solver
//                 above, with or without shrinking);
//   kFormGeneral  Solver::Solve with a general p and start point, one bound C:
//                 one-class and epsilon-SVR;
//   kFormNu       Solver_NU: nu-SVC and nu-SVR.
// The last two read their positions from SvmLaunch::pos_*, run without
// shrinking and write sk_svm_task_solution; see "The general solvers" below.
enum : int { kFormCSvc = 0, kFormGeneral = 1, kFormNu = 2 };

constexpr double kSvmTau = 1e-12;
enum : int { kStLower = 0, kStUpper = 1, kStFree = 2, kStAbsent = 3 };

__device__ __forceinline__ double shfl_xor_f64(double v, int m) { return __shfl_xor(v, m, 64); }

// A value every lane of the wave holds alike, moved to scalar registers (it
// was combined from LDS records in vector registers): what the Solver_NU
// selection carries across step 2, where the largest class has no vector
// register to spare.
__device__ __forceinline__ int uniform_i32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uniform_f32(float v) { return __int_as_float(uniform_i32(__float_as_int(v))); }
__device__ __forceinline__ double uniform_f64(double v) {
  return __hiloint2double(uniform_i32(__double2hiint(v)), uniform_i32(__double2loint(v)));
}

// SHRINK: libsvm's shrinking (Solve(..., shrinking = 1)); its additions are
// described above ("Shrinking") and compiled into that instantiation only.
template <int T, bool SHRINK, int FORM>
__global__ void __launch_bounds__(T) sk_svm_smo_kernel(SvmLaunch L) {
  static_assert(FORM == kFormCSvc || !SHRINK, "shrinking is built for C-SVC only");
  constexpr int E = kSvmElems, W = T / 64, CAP = T * E;
  // How far the loops that combine the waves' records are unrolled.  Whole
  // (W) in the C-SVC instantiations.  The general solvers stop at 8: with all
  // 16 records of the largest class in flight Solver_NU's selection, which
  // combines three sets of them, does not fit the 128 vector registers a
  // workgroup of 1,024 allows.
  constexpr int kGenUnroll = W < 8 ? W : 8, kRecUnroll = FORM == kFormCSvc ? W : kGenUnroll;
  __shared__ double s_val[CAP];
  __shared__ int32_t s_ty[CAP];  // (Gram index << 1) | (y > 0)
  __shared__ RecI s_ri[W];
  __shared__ RecJ s_rj[W];
  __shared__ double s_g2[W];
  __shared__ double s_ub[W], s_lb[W];
  __shared__ int32_t s_nf[W], s_nb[W];
  __shared__ double s_seq[2];
  // kFormNu: the second class's records and reductions
  __shared__ RecI s_rn[W];
  __shared__ double s_g2n[W];
  __shared__ double s_ub2[W], s_lb2[W];
  __shared__ int32_t s_nf2[W];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SvmProb P = L.prob[L.which[blockIdx.x]];
  const int l = FORM == kFormCSvc ? P.n_train : P.n_pos;  // positions
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
    if constexpr (FORM == kFormCSvc) {
      if (k < l) {
        const int t = tr[k];
        tk[e] = t;
        yk[e] = L.ypos[t] ? 1 : -1;
        st[e] = kStLower;
        qd[e] = (float)K[(size_t)t * n + t];
        G[e] = -1.0;
        s_ty[k] = (t << 1) | (yk[e] > 0 ? 1 : 0);
      }
    } else {
      if (k < l) {
        const int ty = L.pos_ty[P.pos_off + k];
        const int t = ty >> 1;
        tk[e] = t;
        yk[e] = (ty & 1) ? 1 : -1;
        al[e] = L.pos_a0[P.pos_off + k];
        st[e] = al[e] >= P.Cp ? kStUpper : al[e] <= 0 ? kStLower : kStFree;
        qd[e] = (float)K[(size_t)t * n + t];
        G[e] = L.pos_p[P.pos_off + k];
        s_ty[k] = ty;
        s_val[k] = st[e] != kStLower ? al[e] : -1.0;
      }
    }
  }
  __syncthreads();
  if constexpr (FORM != kFormCSvc) {
    // the initial gradient (solver.cpp:113-135): G = p, then for every i not
    // at its lower bound in ascending order G[k] += alpha_i Q_i[k], two
    // roundings per term.  The loop over i is uniform (the alphas by position
    // in s_val, -1 at the lower bound); the schedule of reconstruct below.
    for (int i = 0; i < l; ++i) {
      const double a = s_val[i];
      if (a < 0) continue;
      const int ty = s_ty[i];
      const int y_i = (ty & 1) ? 1 : -1;
      const double* __restrict__ ri = K + (size_t)(ty >> 1) * n;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (st[e] != kStAbsent) {
          const float q = (float)((double)(y_i * yk[e]) * ri[tk[e]]);
          G[e] = __dadd_rn(G[e], __dmul_rn(a, (double)q));
        }
    }
    __syncthreads();
  }

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
    // what the selection leaves, to every thread: the pair, its alphas, QD
    // and G, row i's pointer (its entries in qi), and whether to stop
    double gmax = -inf, ai0 = 0.0, gmax2 = -inf, od_min = inf, G_j = 0.0, aj0 = 0.0;
    float qd_i = 0.f, qd_j = 0.f;
    int i = -1, j = -1, y_i = 1;
    const double* __restrict__ ri = K;
    bool optimal;
    if constexpr (FORM != kFormNu) {
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
#pragma unroll kRecUnroll
      for (int w = 0; w < W; ++w) {
        const RecI r = s_ri[w];
        if (r.v > gmax || (r.v == gmax && r.idx > i)) gmax = r.v, i = r.idx, ai0 = r.alpha, qd_i = r.qd;
      }
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
#pragma unroll kRecUnroll
      for (int w = 0; w < W; ++w) {
        const RecJ r = s_rj[w];
        if (r.od < od_min || (r.od == od_min && r.idx > j))
          od_min = r.od, j = r.idx, G_j = r.g, aj0 = r.alpha, qd_j = r.qd;
        const double g = s_g2[w];
        if (g > gmax2) gmax2 = g;
      }
      optimal = __dadd_rn(gmax, gmax2) < P.eps;
    } else {
      // ---- 1 (Solver_NU, solver.cpp:614-641). ip and in: the last maximisers
      // of -G over the y = +1 positions not at the upper bound and of G over
      // the y = -1 positions not at the lower bound.  Two (value, index)
      // arg-max reductions share one butterfly and one barrier, two records
      // per wave.
      double vp = -inf, vn = -inf;
      int xp = -1, xn = -1;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (!live(e)) continue;
        const int k = e * T + tid;
        if (yk[e] > 0) {
          if (st[e] != kStUpper && -G[e] >= vp) vp = -G[e], xp = k;
        } else {
          if (st[e] != kStLower && G[e] >= vn) vn = G[e], xn = k;
        }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const double op = shfl_xor_f64(vp, m), on = shfl_xor_f64(vn, m);
        const int ip_ = __shfl_xor(xp, m, 64), in_ = __shfl_xor(xn, m, 64);
        if (op > vp || (op == vp && ip_ > xp)) vp = op, xp = ip_;
        if (on > vn || (on == vn && in_ > xn)) vn = on, xn = in_;
      }
      // a wave's winner as its record, written by the thread that owns the
      // position (lane 0 when the wave has no candidate)
      auto write_record = [&](RecI* rec, double v, int idx) {
        if (idx >= 0 ? (idx & (T - 1)) == tid : lane == 0) {
          const int slot = idx >= 0 ? idx / T : 0;
          RecI r;
          r.v = v, r.idx = idx, r.alpha = 0.0, r.qd = 0.f;
#pragma unroll
          for (int e = 0; e < E; ++e)
            if (e == slot) r.alpha = al[e], r.qd = qd[e];
          rec[wave] = r;
        }
      };
      write_record(s_ri, vp, xp);
      write_record(s_rn, vn, xn);
      __syncthreads();
      double gmaxp = -inf, gmaxn = -inf, ap0 = 0.0, an0 = 0.0;
      float qd_p = 0.f, qd_n = 0.f;
      int ip = -1, in = -1;
#pragma unroll kGenUnroll
      for (int w = 0; w < W; ++w) {
        const RecI a = s_ri[w], b = s_rn[w];
        if (a.v > gmaxp || (a.v == gmaxp && a.idx > ip)) gmaxp = a.v, ip = a.idx, ap0 = a.alpha, qd_p = a.qd;
        if (b.v > gmaxn || (b.v == gmaxn && b.idx > in)) gmaxn = b.v, in = b.idx, an0 = b.alpha, qd_n = b.qd;
      }
      gmaxp = uniform_f64(gmaxp), gmaxn = uniform_f64(gmaxn), ap0 = uniform_f64(ap0), an0 = uniform_f64(an0);
      qd_p = uniform_f32(qd_p), qd_n = uniform_f32(qd_n), ip = uniform_i32(ip), in = uniform_i32(in);
      // rows ip and in: step 2 reads Q_ip[k] at the y = +1 positions only and
      // Q_in[k] at the y = -1 positions only (y_i y_k = +1 in both), so every
      // position gathers one entry, from its own class's row; a class whose
      // index is -1 is skipped
      const double* __restrict__ rp = ip >= 0 ? K + (size_t)uniform_i32(s_ty[ip] >> 1) * n : K;
      const double* __restrict__ rn = in >= 0 ? K + (size_t)uniform_i32(s_ty[in] >> 1) * n : K;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (live(e) && (yk[e] > 0 ? ip : in) >= 0) qi[e] = (float)(yk[e] > 0 ? rp : rn)[tk[e]];

      // ---- 2 (solver.cpp:643-693). j: the last minimiser of the objective's
      // decrease over both classes, each against its own class's maximiser;
      // Gmaxp2 and Gmaxn2 ride along
      double od = inf, g2p = -inf, g2n = -inf;
      int jdx = -1;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (!live(e)) continue;
        double gd;
        float qf;
        if (yk[e] > 0) {
          if (st[e] == kStLower) continue;
          gd = __dadd_rn(gmaxp, G[e]);
          if (G[e] >= g2p) g2p = G[e];
          if (!(gd > 0)) continue;
          qf = __fsub_rn(__fadd_rn(qd_p, qd[e]), __fmul_rn(2.f, qi[e]));
        } else {
          if (st[e] == kStUpper) continue;
          gd = __dsub_rn(gmaxn, G[e]);
          if (-G[e] >= g2n) g2n = -G[e];
          if (!(gd > 0)) continue;
          qf = __fsub_rn(__fadd_rn(qd_n, qd[e]), __fmul_rn(2.f, qi[e]));
        }
        const double qc = (double)qf;
        const double od_e = -__ddiv_rn(__dmul_rn(gd, gd), qc > 0 ? qc : kSvmTau);
        if (od_e <= od) od = od_e, jdx = e * T + tid;
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const double oo = shfl_xor_f64(od, m);
        const int oj = __shfl_xor(jdx, m, 64);
        const double ogp = shfl_xor_f64(g2p, m), ogn = shfl_xor_f64(g2n, m);
        if (oo < od || (oo == od && oj > jdx)) od = oo, jdx = oj;
        if (ogp > g2p) g2p = ogp;
        if (ogn > g2n) g2n = ogn;
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
      if (lane == 0) s_g2[wave] = g2p, s_g2n[wave] = g2n;
      __syncthreads();
      double gmaxp2 = -inf, gmaxn2 = -inf;
#pragma unroll kGenUnroll
      for (int w = 0; w < W; ++w) {
        const RecJ r = s_rj[w];
        if (r.od < od_min || (r.od == od_min && r.idx > j))
          od_min = r.od, j = r.idx, G_j = r.g, aj0 = r.alpha, qd_j = r.qd;
        if (s_g2[w] > gmaxp2) gmaxp2 = s_g2[w];
        if (s_g2n[w] > gmaxn2) gmaxn2 = s_g2n[w];
      }
      od_min = uniform_f64(od_min), G_j = uniform_f64(G_j), aj0 = uniform_f64(aj0), qd_j = uniform_f32(qd_j);
      j = uniform_i32(j), gmaxp2 = uniform_f64(gmaxp2), gmaxn2 = uniform_f64(gmaxn2);
      const double sp = __dadd_rn(gmaxp, gmaxp2), sn = __dadd_rn(gmaxn, gmaxn2);
      optimal = (sp < sn ? sn : sp) < P.eps;  // std::max (solver.cpp:695)
      // i comes from the class of the chosen j (:698-701): qi holds row i at
      // the positions of that class, and step 4 gathers it at the others.
      // No j: the reference reads y[-1]; here SK_SVM_NO_PAIR.
      if (j >= 0) {
        if (s_ty[j] & 1) i = ip, y_i = 1, gmax = gmaxp, ai0 = ap0, qd_i = qd_p, ri = rp;
        else i = in, y_i = -1, gmax = gmaxn, ai0 = an0, qd_i = qd_n, ri = rn;
      }
    }

    // ---- 3. stop, or update alpha_i and alpha_j (every thread, same values)
    if constexpr (!SHRINK) {
      if (optimal) break;
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
      if (optimal) {
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
    if constexpr (FORM == kFormNu) {
      // the rest of row i: the positions of the other class (y_i y_k = -1)
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (live(e) && yk[e] != y_i) qi[e] = (float)((double)(y_i * yk[e]) * ri[tk[e]]);
    }
    const float q_ij = (float)((double)(y_i * y_j) * ri[tyj >> 1]);
    const double G_i = y_i > 0 ? -gmax : gmax;
    // the general solvers have one bound; Solver_NU pairs within a class
    const double Ci = FORM != kFormCSvc || y_i > 0 ? P.Cp : P.Cn, Cj = FORM != kFormCSvc || y_j > 0 ? P.Cp : P.Cn;
    double ai = ai0, aj = aj0;
    if (FORM != kFormNu && y_i != y_j) {
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

  if constexpr (FORM == kFormCSvc) {
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
  } else {
    // ---- the general solvers' epilogue.  rho (and r) as calculate_rho
    // (solver.cpp:554-592; Solver_NU :799-848): the sums over the free
    // positions are added by one thread from LDS in position order (+0.0 for
    // the others changes no bit), the bounds and counts by exact reductions.
    // Class 1 is y = +1.  The plain solver keeps y G in one class's slots.
    double ub1 = inf, lb1 = -inf, ub2 = inf, lb2 = -inf;
    int nf1 = 0, nf2 = 0, nb = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (st[e] == kStAbsent) continue;
      if (st[e] == kStUpper) ++nb;
      if constexpr (FORM == kFormNu) {
        if (yk[e] > 0) {
          if (st[e] == kStUpper) lb1 = G[e] > lb1 ? G[e] : lb1;
          else if (st[e] == kStLower) ub1 = G[e] < ub1 ? G[e] : ub1;
          else ++nf1;
        } else {
          if (st[e] == kStUpper) lb2 = G[e] > lb2 ? G[e] : lb2;
          else if (st[e] == kStLower) ub2 = G[e] < ub2 ? G[e] : ub2;
          else ++nf2;
        }
      } else {
        const double yg = yk[e] > 0 ? G[e] : -G[e];
        if (st[e] == kStUpper) {
          if (yk[e] < 0) ub1 = yg < ub1 ? yg : ub1;
          else lb1 = yg > lb1 ? yg : lb1;
        } else if (st[e] == kStLower) {
          if (yk[e] > 0) ub1 = yg < ub1 ? yg : ub1;
          else lb1 = yg > lb1 ? yg : lb1;
        } else {
          ++nf1;
        }
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double ou = shfl_xor_f64(ub1, m), ol = shfl_xor_f64(lb1, m);
      ub1 = ou < ub1 ? ou : ub1;
      lb1 = ol > lb1 ? ol : lb1;
      nf1 += __shfl_xor(nf1, m, 64);
      nb += __shfl_xor(nb, m, 64);
      if constexpr (FORM == kFormNu) {
        const double ou2 = shfl_xor_f64(ub2, m), ol2 = shfl_xor_f64(lb2, m);
        ub2 = ou2 < ub2 ? ou2 : ub2;
        lb2 = ol2 > lb2 ? ol2 : lb2;
        nf2 += __shfl_xor(nf2, m, 64);
      }
    }
    if (lane == 0) {
      s_ub[wave] = ub1, s_lb[wave] = lb1, s_nf[wave] = nf1, s_nb[wave] = nb;
      if constexpr (FORM == kFormNu) s_ub2[wave] = ub2, s_lb2[wave] = lb2, s_nf2[wave] = nf2;
    }
    // the sums over the free positions, one pass per class: every thread
    // writes its term (+0.0 unless free and of the class), thread 0 adds them
    // in position order
#pragma unroll
    for (int c = 0; c < (FORM == kFormNu ? 2 : 1); ++c) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (st[e] == kStAbsent) continue;
        double f = 0.0;
        if constexpr (FORM == kFormNu) {
          if (st[e] == kStFree && (yk[e] > 0) == (c == 0)) f = G[e];
        } else {
          if (st[e] == kStFree) f = yk[e] > 0 ? G[e] : -G[e];
        }
        s_val[e * T + tid] = f;
      }
      __syncthreads();
      if (tid == 0) {
        double sum = 0.0;
        for (int k = 0; k < l; ++k) sum = __dadd_rn(sum, s_val[k]);
        s_seq[c] = sum;
      }
      __syncthreads();
    }
    ub1 = inf, lb1 = -inf, ub2 = inf, lb2 = -inf, nf1 = 0, nf2 = 0, nb = 0;
#pragma unroll 1  // runs once; unrolled, its 7 W loads push the largest class into scratch
    for (int w = 0; w < W; ++w) {
      ub1 = s_ub[w] < ub1 ? s_ub[w] : ub1;
      lb1 = s_lb[w] > lb1 ? s_lb[w] : lb1;
      nf1 += s_nf[w];
      nb += s_nb[w];
      if constexpr (FORM == kFormNu) {
        ub2 = s_ub2[w] < ub2 ? s_ub2[w] : ub2;
        lb2 = s_lb2[w] > lb2 ? s_lb2[w] : lb2;
        nf2 += s_nf2[w];
      }
    }
    const double r1 = nf1 > 0 ? __ddiv_rn(s_seq[0], (double)nf1) : __ddiv_rn(__dadd_rn(ub1, lb1), 2.0);
    double rho = r1, r = 0.0;
    if constexpr (FORM == kFormNu) {
      const double r2 = nf2 > 0 ? __ddiv_rn(s_seq[1], (double)nf2) : __ddiv_rn(__dadd_rn(ub2, lb2), 2.0);
      r = __ddiv_rn(__dadd_rn(r1, r2), 2.0);
      rho = __ddiv_rn(__dsub_rn(r1, r2), 2.0);
    }
    // ---- obj = sum alpha (G + p) / 2, in position order
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (st[e] != kStAbsent)
        s_val[e * T + tid] = __dmul_rn(al[e], __dadd_rn(G[e], L.pos_p[P.pos_off + e * T + tid]));
    __syncthreads();
    if (tid == 0) {
      double sum = 0.0;
      for (int k = 0; k < l; ++k) sum = __dadd_rn(sum, s_val[k]);
      s_seq[0] = sum;
    }
    __syncthreads();
    double obj = __ddiv_rn(s_seq[0], 2.0);
    // ---- what svm_train_one keeps (svm.cpp:116-122, :188, :229): the
    // coefficients by training example in s_val, rho and obj scaled for nu-SVC
    const int lt = P.n_train;
    if (P.svm_type == SK_SVM_EPSILON_SVR || P.svm_type == SK_SVM_NU_SVR) {
      // alpha_k - alpha_{k+l}: both halves through LDS
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (st[e] != kStAbsent) s_val[e * T + tid] = al[e];
      __syncthreads();
      double c[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int k = e * T + tid;
        c[e] = k < lt ? __dsub_rn(s_val[k], s_val[k + lt]) : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (e * T + tid < lt) s_val[e * T + tid] = c[e];
    } else if (P.svm_type == SK_SVM_NU_SVC) {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (st[e] != kStAbsent) s_val[e * T + tid] = __dmul_rn(al[e], __ddiv_rn((double)yk[e], r));
      rho = __ddiv_rn(rho, r);
      obj = __ddiv_rn(obj, __dmul_rn(r, r));
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (st[e] != kStAbsent) s_val[e * T + tid] = al[e];
    }
    __syncthreads();
    if (tid == 0) {
      sk_svm_task_solution S;
      S.rho = rho;
      S.obj = obj;
      S.iterations = iter;
      S.status = status;
      S.n_free = nf1 + nf2;
      S.n_bound = nb;
      S.r = r;
      L.tsol[L.which[blockIdx.x]] = S;
    }
    for (int k = tid; k < lt; k += T) L.alpha[P.train_off + k] = s_val[k];
    // ---- decision values of the test list: one wave per test example
    for (int q = wave; q < P.n_test; q += W) {
      const double* __restrict__ rs = K + (size_t)L.test[P.test_off + q] * n;
      double sum = 0.0;
      for (int a = lane; a < lt; a += 64) {
        const double c = s_val[a];
        if (c != 0.0) sum = __dadd_rn(sum, __dmul_rn(c, rs[s_ty[a] >> 1]));
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) sum = __dadd_rn(sum, shfl_xor_f64(sum, m));
      if (lane == 0) L.dec[P.test_off + q] = __dsub_rn(sum, rho);
    }
  }
}

template <int T>
hipError_t launch_class(const SvmLaunch& L, int form, bool shrinking, int grid, hipStream_t st) {
  if (form == kFormGeneral)
    hipLaunchKernelGGL((sk_svm_smo_kernel<T, false, kFormGeneral>), dim3(grid), dim3(T), 0, st, L);
  else if (form == kFormNu)
    hipLaunchKernelGGL((sk_svm_smo_kernel<T, false, kFormNu>), dim3(grid), dim3(T), 0, st, L);
  else if (shrinking)
    hipLaunchKernelGGL((sk_svm_smo_kernel<T, true, kFormCSvc>), dim3(grid), dim3(T), 0, st, L);
  else
    hipLaunchKernelGGL((sk_svm_smo_kernel<T, false, kFormCSvc>), dim3(grid), dim3(T), 0, st, L);
  return hipGetLastError();
}

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// One call's host images: the labels' signs, the lists concatenated, the
// descriptors and, for the general solvers, the positions; form[p] is the
// kernel family of problem p.
struct SvmBatch {
  std::vector<signed char> ypos;
  std::vector<int32_t> train, test, pos_ty;
  std::vector<double> pos_p, pos_a0;
  std::vector<SvmProb> prob;
  std::vector<int> form;
};

// The images of a call's checked jobs.  The C-SVC family reads its training
// list and ypos; the general families get their positions.
SvmBatch svm_build_batch(const double* targets, int32_t n, const std::vector<SvmJob>& jobs, int64_t sum_train,
                         int64_t sum_test) {
  SvmBatch B;
  B.ypos.assign(n, 0);
  if (targets)
    for (int32_t k = 0; k < n; ++k) B.ypos[k] = targets[k] > 0 ? 1 : 0;
  B.train.resize((size_t)sum_train), B.test.resize((size_t)sum_test);
  B.prob.resize(jobs.size());
  B.form.resize(jobs.size());
  int32_t to = 0, so = 0;
  for (size_t p = 0; p < jobs.size(); ++p) {
    const SvmJob& J = jobs[p];
    SvmProb& D = B.prob[p];
    D.max_iter = J.max_iter;
    D.eps = J.eps;
    D.train_off = to, D.n_train = J.n_train, D.test_off = so, D.n_test = J.n_test;
    D.svm_type = J.svm_type;
    if (J.svm_type == SK_SVM_C_SVC) {
      B.form[p] = kFormCSvc;
      D.Cp = J.Cp, D.Cn = J.Cn;
      D.pos_off = 0, D.n_pos = 0;
    } else {
      B.form[p] = svm_type_is_nu(J.svm_type) ? kFormNu : kFormGeneral;
      D.pos_off = (int32_t)B.pos_ty.size();
      D.n_pos = svm_task_positions(targets, J, B.pos_ty, B.pos_p, B.pos_a0, &D.Cp, &D.Cn);
    }
    std::memcpy(B.train.data() + to, J.train, (size_t)J.n_train * 4);
    if (J.n_test) std::memcpy(B.test.data() + so, J.test, (size_t)J.n_test * 4);
    to += J.n_train;
    so += J.n_test;
  }
  return B;
}

constexpr int kSvmForms = 3;

#define SK_SVM_HIP(expr)                                                                          \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess)                                                                         \
      return ctx_fail(ctx, SK_ERR_HIP, std::string(who) + ": " #expr ": " + hipGetErrorString(_e)); \
  } while (0)

// Upload, one launch per (family, size class) in use, download.  alpha_out:
// sum of n_train values (alphas, or the general solvers' coefficients);
// sol_out / tsol_out: n_problems records each, written for the problems of
// the C-SVC family / of the general families (either may be null when no
// problem of its kind is in the batch).
int svm_run_batch(sk_context* ctx, const char* who, const double* gram, int32_t n, const SvmBatch& B, bool shrinking,
                  double* alpha_out, double* dec_out, sk_svm_solution* sol_out, sk_svm_task_solution* tsol_out,
                  sk_svm_shrink_info* info_out) {
  const int n_problems = (int)B.prob.size();
  const size_t sum_train = B.train.size(), sum_test = B.test.size(), sum_pos = B.pos_ty.size();
  std::vector<int32_t> which[kSvmForms][kSvmClasses];
  for (int p = 0; p < n_problems; ++p) {
    const int positions = B.form[p] == kFormCSvc ? B.prob[p].n_train : B.prob[p].n_pos;
    int c = 0;
    while (positions > kSvmThreads[c] * kSvmElems) ++c;
    which[B.form[p]][c].push_back(p);
  }
  std::vector<int32_t> which_all;
  int32_t which_off[kSvmForms][kSvmClasses];
  for (int f = 0; f < kSvmForms; ++f)
    for (int c = 0; c < kSvmClasses; ++c) {
      which_off[f][c] = (int32_t)which_all.size();
      which_all.insert(which_all.end(), which[f][c].begin(), which[f][c].end());
    }

  SK_SVM_HIP(hipSetDevice(ctx_device(ctx)));
  // a fresh timing set for the launch events below, collected before this
  // call returns (lev_collect), so no call_finish: the call is synchronous and
  // stages nothing.  On an asynchronous context call_begin also advances the
  // staging ring by one slot, which this call leaves empty (sk_bpla_gradients
  // does the same).
  SK_SVM_HIP(call_begin(ctx));
  hipStream_t S = ctx_stream(ctx);
  // one device arena
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) & ~(size_t)255;
    return at;
  };
  const size_t o_gram = take((size_t)n * n * 8), o_y = take((size_t)n), o_tr = take(sum_train * 4),
               o_ts = take(sum_test * 4), o_pr = take((size_t)n_problems * sizeof(SvmProb)),
               o_wh = take((size_t)n_problems * 4), o_al = take(sum_train * 8), o_de = take(sum_test * 8),
               o_so = take((size_t)n_problems * sizeof(sk_svm_solution)),
               o_in = take((size_t)n_problems * sizeof(sk_svm_shrink_info)), o_pt = take(sum_pos * 4),
               o_pp = take(sum_pos * 8), o_pa = take(sum_pos * 8),
               o_ts2 = take((size_t)n_problems * sizeof(sk_svm_task_solution));
  DevBuf buf;
  if (hipMalloc(&buf.p, off) != hipSuccess) {
    (void)hipGetLastError();
    return ctx_fail(ctx, SK_ERR_ALLOC, std::string(who) + ": device memory for the Gram and the lists");
  }
  char* base = static_cast<char*>(buf.p);
  auto up = [&](size_t at, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(base + at, src, bytes, hipMemcpyHostToDevice, S) : hipSuccess;
  };
  SK_SVM_HIP(up(o_gram, gram, (size_t)n * n * 8));
  SK_SVM_HIP(up(o_y, B.ypos.data(), (size_t)n));
  SK_SVM_HIP(up(o_tr, B.train.data(), sum_train * 4));
  SK_SVM_HIP(up(o_ts, B.test.data(), sum_test * 4));
  SK_SVM_HIP(up(o_pr, B.prob.data(), (size_t)n_problems * sizeof(SvmProb)));
  SK_SVM_HIP(up(o_wh, which_all.data(), (size_t)n_problems * 4));
  SK_SVM_HIP(up(o_pt, B.pos_ty.data(), sum_pos * 4));
  SK_SVM_HIP(up(o_pp, B.pos_p.data(), sum_pos * 8));
  SK_SVM_HIP(up(o_pa, B.pos_a0.data(), sum_pos * 8));
  SvmLaunch L;
  L.gram = reinterpret_cast<const double*>(base + o_gram);
  L.n = n;
  L.ypos = reinterpret_cast<const signed char*>(base + o_y);
  L.train = reinterpret_cast<const int32_t*>(base + o_tr);
  L.test = reinterpret_cast<const int32_t*>(base + o_ts);
  L.prob = reinterpret_cast<const SvmProb*>(base + o_pr);
  L.alpha = reinterpret_cast<double*>(base + o_al);
  L.dec = reinterpret_cast<double*>(base + o_de);
  L.sol = reinterpret_cast<sk_svm_solution*>(base + o_so);
  L.info = reinterpret_cast<sk_svm_shrink_info*>(base + o_in);
  L.pos_ty = reinterpret_cast<const int32_t*>(base + o_pt);
  L.pos_p = reinterpret_cast<const double*>(base + o_pp);
  L.pos_a0 = reinterpret_cast<const double*>(base + o_pa);
  L.tsol = reinterpret_cast<sk_svm_task_solution*>(base + o_ts2);
  // largest class first: its workgroups run longest
  for (int c = kSvmClasses - 1; c >= 0; --c)
    for (int f = 0; f < kSvmForms; ++f) {
      if (which[f][c].empty()) continue;
      L.which = reinterpret_cast<const int32_t*>(base + o_wh) + which_off[f][c];
      const int grid = (int)which[f][c].size();
      SK_SVM_HIP(lev_mark(ctx, S));
      if (c == 0) SK_SVM_HIP(launch_class<kSvmThreads[0]>(L, f, shrinking, grid, S));
      if (c == 1) SK_SVM_HIP(launch_class<kSvmThreads[1]>(L, f, shrinking, grid, S));
      if (c == 2) SK_SVM_HIP(launch_class<kSvmThreads[2]>(L, f, shrinking, grid, S));
      SK_SVM_HIP(lev_mark(ctx, S));
    }
  SK_SVM_HIP(hipMemcpyAsync(alpha_out, base + o_al, sum_train * 8, hipMemcpyDeviceToHost, S));
  if (sum_test) SK_SVM_HIP(hipMemcpyAsync(dec_out, base + o_de, sum_test * 8, hipMemcpyDeviceToHost, S));
  if (sol_out)
    SK_SVM_HIP(hipMemcpyAsync(sol_out, base + o_so, (size_t)n_problems * sizeof(sk_svm_solution),
                              hipMemcpyDeviceToHost, S));
  if (tsol_out)
    SK_SVM_HIP(hipMemcpyAsync(tsol_out, base + o_ts2, (size_t)n_problems * sizeof(sk_svm_task_solution),
                              hipMemcpyDeviceToHost, S));
  if (info_out && shrinking)
    SK_SVM_HIP(hipMemcpyAsync(info_out, base + o_in, (size_t)n_problems * sizeof(sk_svm_shrink_info),
                              hipMemcpyDeviceToHost, S));
  SK_SVM_HIP(hipStreamSynchronize(S));
  SK_SVM_HIP(lev_collect(ctx));
  return SK_OK;
}

#undef SK_SVM_HIP

}  // namespace
}  // namespace sk

extern "C" int sk_svm_train_batch_ex(sk_context* ctx, const double* gram, int32_t n, const double* labels,
                                     const sk_svm_problem* problems, int32_t n_problems, int32_t shrinking,
                                     double* alpha_out, double* dec_out, sk_svm_solution* solutions,
                                     sk_svm_shrink_info* info) {
  if (!ctx) return SK_ERR_INVALID;
  try {
    sk::lev_reset(ctx);
    std::string err;
    int64_t sum_train = 0, sum_test = 0;
    const std::vector<sk::SvmJob> jobs = sk::svm_jobs(problems, n_problems);
    const int rc = sk::svm_check_jobs(sk::kSvmTrainBatch, gram, n, labels, jobs, n_problems, alpha_out, dec_out,
                                      solutions, true, &sum_train, &sum_test, err);
    if (rc) return sk::ctx_fail(ctx, rc, err);
    if (n_problems == 0) return SK_OK;
    if (sum_train > INT32_MAX || sum_test > INT32_MAX)
      return sk::ctx_fail(ctx, SK_ERR_UNSUPPORTED, "sk_svm_train_batch: over 2^31 list entries in one call");

    const sk::SvmBatch B = sk::svm_build_batch(labels, n, jobs, sum_train, sum_test);
    const int rr = sk::svm_run_batch(ctx, "sk_svm_train_batch", gram, n, B, shrinking != 0, alpha_out, dec_out,
                                     solutions, nullptr, info);
    if (rr) return rr;
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

extern "C" int sk_svm_solve_batch(sk_context* ctx, const double* gram, int32_t n, const double* targets,
                                  const sk_svm_task* tasks, int32_t n_tasks, double* coef_out, double* dec_out,
                                  sk_svm_task_solution* solutions) {
  if (!ctx) return SK_ERR_INVALID;
  try {
    sk::lev_reset(ctx);
    std::string err;
    int64_t sum_train = 0, sum_test = 0;
    const std::vector<sk::SvmJob> jobs = sk::svm_jobs(tasks, n_tasks);
    const int rc = sk::svm_check_jobs(sk::kSvmSolveBatch, gram, n, targets, jobs, n_tasks, coef_out, dec_out,
                                      solutions, true, &sum_train, &sum_test, err);
    if (rc) return sk::ctx_fail(ctx, rc, err);
    if (n_tasks == 0) return SK_OK;
    if (2 * sum_train > INT32_MAX || sum_test > INT32_MAX)
      return sk::ctx_fail(ctx, SK_ERR_UNSUPPORTED, "sk_svm_solve_batch: over 2^31 list entries in one call");

    // a C-SVC task is sk_svm_train_batch's problem with Cp = Cn = C, and runs its kernel
    const sk::SvmBatch B = sk::svm_build_batch(targets, n, jobs, sum_train, sum_test);
    bool any_csvc = false;
    for (int form : B.form) any_csvc |= form == sk::kFormCSvc;
    std::vector<sk_svm_solution> csvc(any_csvc ? n_tasks : 0);
    const int rr = sk::svm_run_batch(ctx, "sk_svm_solve_batch", gram, n, B, false, coef_out, dec_out,
                                     any_csvc ? csvc.data() : nullptr, solutions, nullptr);
    if (rr) return rr;
    // C-SVC: coef = alpha y (svm.cpp:66-67), the solution as sk_svm_train_batch gives it
    for (int p = 0; p < n_tasks; ++p) {
      if (tasks[p].svm_type != SK_SVM_C_SVC) continue;
      double* c = coef_out + B.prob[p].train_off;
      for (int k = 0; k < tasks[p].n_train; ++k) c[k] *= targets[tasks[p].train[k]] > 0 ? 1 : -1;
      const sk_svm_solution& s = csvc[p];
      solutions[p] = sk_svm_task_solution{s.rho, s.obj, s.iterations, s.status, s.n_free, s.n_bound, 0.0};
    }
    return SK_OK;
  } catch (const std::bad_alloc&) {
    return sk::ctx_fail(ctx, SK_ERR_ALLOC, "sk_svm_solve_batch: host memory");
  }
}
