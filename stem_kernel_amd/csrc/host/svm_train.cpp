// Portions (the SMO iteration below keeps libsvm's operation order, and so its
// structure, for bit-compatible alphas) derive from LIBSVM:
//   Copyright (c) 2000-2007 Chih-Chung Chang and Chih-Jen Lin.
//   All rights reserved.
//   Redistribution and use in source and binary forms, with or without
//   modification, are permitted provided that the following conditions are
//   met: 1. Redistributions of source code must retain the above copyright
//   notice, this list of conditions and the following disclaimer.
//   2. Redistributions in binary form must reproduce the above copyright
//   notice, this list of conditions and the following disclaimer in the
//   documentation and/or other materials provided with the distribution.
//   3. Neither name of copyright holders nor the names of its contributors
//   may be used to endorse or promote products derived from this software
//   without specific prior written permission.
//   THIS SOFTWARE IS PROVIDED BY THE COPYRIGHT HOLDERS AND CONTRIBUTORS "AS
//   IS" AND ANY EXPRESS OR IMPLIED WARRANTIES, INCLUDING, BUT NOT LIMITED TO,
//   THE IMPLIED WARRANTIES OF MERCHANTABILITY AND FITNESS FOR A PARTICULAR
//   PURPOSE ARE DISCLAIMED.  IN NO EVENT SHALL THE REGENTS OR CONTRIBUTORS BE
//   LIABLE FOR ANY DIRECT, INDIRECT, INCIDENTAL, SPECIAL, EXEMPLARY, OR
//   CONSEQUENTIAL DAMAGES (INCLUDING, BUT NOT LIMITED TO, PROCUREMENT OF
//   SUBSTITUTE GOODS OR SERVICES; LOSS OF USE, DATA, OR PROFITS; OR BUSINESS
//   INTERRUPTION) HOWEVER CAUSED AND ON ANY THEORY OF LIABILITY, WHETHER IN
//   CONTRACT, STRICT LIABILITY, OR TORT (INCLUDING NEGLIGENCE OR OTHERWISE)
//   ARISING IN ANY WAY OUT OF THE USE OF THIS SOFTWARE, EVEN IF ADVISED OF
//   THE POSSIBILITY OF SUCH DAMAGE.
//
// Two-class C-SVC training on a precomputed Gram: the reference's SMO solver,
// without shrinking (solve_one) and with it (solve_one_shrink, which lists
// what it adds), restated from the published algorithm (Fan, Chen and
// Lin, JMLR 6 (2005), working-set selection 3):
//   Solver::Solve            libsvm/solver.cpp:81-349   (start :113-135, the
//                            two-variable update :180-265, G update :272-275,
//                            obj :314-321)
//   select_working_set       solver.cpp:352-451
//   calculate_rho            solver.cpp:554-592
//   update_alpha_status      libsvm/solver.h:67-74
//   SVC_Q                    libsvm/qmatrix.cpp:339-362 (QD, get_Q: float)
//   kernel_precomputed       qmatrix.cpp:331-336
//   solve_c_svc              libsvm/svm.cpp:38-71       (p = -1, alpha = 0, y)
//   svm_train / svm_predict  optimizer/gradient.cpp:208-246, :248-278
//   svm_save_model           svm.cpp:1201-1286, svm_group_classes :611-666
// With the active set whole, reconstruct_gradient and the second selection
// change nothing (solver.cpp:154-165), G_bar is never read, and the Q cache
// (a store of rows, qmatrix.cpp:37-60) does not touch a value.
//
// Next to C-SVC, GenSmo below restates the general Solve and Solver_NU without
// shrinking for the other four formulations of svm_train_one
// (libsvm/svm.cpp:245-300), set up as the reference's solve_* functions do:
//   solve_nu_svc :73-126, solve_one_class :128-158, solve_epsilon_svr :160-196,
//   solve_nu_svr :198-234; Solver_NU::select_working_set solver.cpp:595-705,
//   Solver_NU::calculate_rho :799-848; ONE_CLASS_Q / SVR_Q qmatrix.cpp:382-475;
//   svm_check_parameter svm.cpp:1499-1615; the one-class / regression model
//   svm.cpp:677-717.
// Shrinking for those four (Solver_NU::do_shrinking included) is not built.
//
// This file is the CPU path of sk_svm_train_batch[_ex] and sk_svm_solve_batch,
// what tests/golden/svm_train.json, svm_train_shrink.json and
// svm_formulations.json pin, and what the GPU kernel (kernels/svm_smo.hip) is
// compared with.  Built with -ffp-contract=off: the G update has four
// roundings.
#include "svm_train.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <limits>
#include <system_error>
#include <thread>
#include <vector>

namespace {

constexpr double kTau = 1e-12;
constexpr double kInf = std::numeric_limits<double>::infinity();
enum : char { kLower, kUpper, kFree };

struct Smo {
  const double* K;
  size_t n;
  const int32_t* t;
  int l;
  double Cp, Cn;
  std::vector<signed char> y;
  std::vector<float> QD, Qi, Qj;
  std::vector<double> G;
  std::vector<char> st;
  double* alpha;

  double bound(int k) const { return y[k] > 0 ? Cp : Cn; }
  void status(int k) { st[k] = alpha[k] >= bound(k) ? kUpper : alpha[k] <= 0 ? kLower : kFree; }
  // row i of Q: the int product of the labels times the double, rounded to float
  void row(int i, std::vector<float>& q) const {
    const double* r = K + (size_t)t[i] * n;
    const int yi = y[i];
    for (int k = 0; k < l; ++k) q[k] = (float)(yi * y[k] * r[t[k]]);
  }
};

// The clipped two-variable update (solver.cpp:180-265) on alpha_i, alpha_j:
// opposite labels or equal ones; quad_coef in float arithmetic.
void update_pair(bool opposite, float Qii, float Qjj, float Qij, double Gi, double Gj, double Ci, double Cj,
                 double& ai, double& aj) {
  if (opposite) {
    const float qf = Qii + Qjj + 2 * Qij;
    double qc = qf;
    if (qc <= 0) qc = kTau;
    const double delta = (-Gi - Gj) / qc;
    const double diff = ai - aj;
    ai += delta;
    aj += delta;
    if (diff > 0) {
      if (aj < 0) aj = 0, ai = diff;
    } else {
      if (ai < 0) ai = 0, aj = -diff;
    }
    if (diff > Ci - Cj) {
      if (ai > Ci) ai = Ci, aj = Ci - diff;
    } else {
      if (aj > Cj) aj = Cj, ai = Cj + diff;
    }
  } else {
    const float qf = Qii + Qjj - 2 * Qij;
    double qc = qf;
    if (qc <= 0) qc = kTau;
    const double delta = (Gi - Gj) / qc;
    const double sum = ai + aj;
    ai -= delta;
    aj += delta;
    if (sum > Ci) {
      if (ai > Ci) ai = Ci, aj = sum - Ci;
    } else {
      if (aj < 0) aj = 0, ai = sum;
    }
    if (sum > Cj) {
      if (aj > Cj) aj = Cj, ai = sum - Cj;
    } else {
      if (ai < 0) ai = 0, aj = sum;
    }
  }
}

void solve_one(const double* K, int32_t n, const double* labels, const sk_svm_problem& P, double* alpha,
               double* dec, sk_svm_solution& S) {
  Smo s;
  s.K = K;
  s.n = (size_t)n;
  s.t = P.train;
  const int l = s.l = P.n_train;
  s.Cp = P.Cp;
  s.Cn = P.Cn;
  s.alpha = alpha;
  s.y.resize(l);
  s.QD.resize(l);
  s.Qi.resize(l);
  s.Qj.resize(l);
  s.G.assign(l, -1.0);
  s.st.assign(l, kLower);
  for (int k = 0; k < l; ++k) {
    s.y[k] = labels[s.t[k]] > 0 ? +1 : -1;
    s.QD[k] = (float)K[(size_t)s.t[k] * s.n + s.t[k]];
    alpha[k] = 0.0;
  }
  const std::vector<signed char>& y = s.y;
  std::vector<double>& G = s.G;
  const std::vector<float>&QD = s.QD, &Qi = s.Qi, &Qj = s.Qj;

  int64_t iter = 0;
  int32_t status = SK_SVM_CONVERGED;
  for (;;) {
    // i: the last maximiser of -y G over I_up
    double gmax = -kInf, gmax2 = -kInf, od_min = kInf;
    int i = -1, j = -1;
    for (int k = 0; k < l; ++k) {
      if (y[k] > 0) {
        if (s.st[k] != kUpper && -G[k] >= gmax) gmax = -G[k], i = k;
      } else {
        if (s.st[k] != kLower && G[k] >= gmax) gmax = G[k], i = k;
      }
    }
    if (i >= 0) s.row(i, s.Qi);
    // j: the last minimiser of the objective's decrease over I_low
    for (int k = 0; k < l; ++k) {
      double gd;
      float qf;
      if (y[k] > 0) {
        if (s.st[k] == kLower) continue;
        gd = gmax + G[k];
        if (G[k] >= gmax2) gmax2 = G[k];
        if (!(gd > 0)) continue;
        qf = Qi[i] + QD[k] - 2 * y[i] * Qi[k];  // float arithmetic
      } else {
        if (s.st[k] == kUpper) continue;
        gd = gmax - G[k];
        if (-G[k] >= gmax2) gmax2 = -G[k];
        if (!(gd > 0)) continue;
        qf = Qi[i] + QD[k] + 2 * y[i] * Qi[k];
      }
      const double qc = qf;
      const double od = qc > 0 ? -(gd * gd) / qc : -(gd * gd) / kTau;
      if (od <= od_min) od_min = od, j = k;
    }
    if (gmax + gmax2 < P.eps) break;
    if (i < 0 || j < 0) {
      status = SK_SVM_NO_PAIR;
      break;
    }
    if (iter == P.max_iter) {
      status = SK_SVM_NOT_CONVERGED;
      break;
    }
    ++iter;
    s.row(j, s.Qj);

    const double Ci = s.bound(i), Cj = s.bound(j);
    const double ai0 = alpha[i], aj0 = alpha[j];
    update_pair(y[i] != y[j], Qi[i], Qj[j], Qi[j], G[i], G[j], Ci, Cj, alpha[i], alpha[j]);
    const double dai = alpha[i] - ai0, daj = alpha[j] - aj0;
    for (int k = 0; k < l; ++k) G[k] += Qi[k] * dai + Qj[k] * daj;
    s.status(i);
    s.status(j);
  }

  // rho: the mean of y G over the free variables, else the bounds' midpoint
  int n_free = 0, n_bound = 0;
  double ub = kInf, lb = -kInf, sum_free = 0;
  for (int k = 0; k < l; ++k) {
    const double yg = y[k] * G[k];
    if (s.st[k] == kUpper) {
      ++n_bound;
      if (y[k] < 0) ub = std::min(ub, yg);
      else lb = std::max(lb, yg);
    } else if (s.st[k] == kLower) {
      if (y[k] > 0) ub = std::min(ub, yg);
      else lb = std::max(lb, yg);
    } else {
      ++n_free;
      sum_free += yg;
    }
  }
  S.rho = n_free > 0 ? sum_free / n_free : (ub + lb) / 2;
  double v = 0;
  for (int k = 0; k < l; ++k) v += alpha[k] * (G[k] + -1.0);
  S.obj = v / 2;
  S.iterations = iter;
  S.status = status;
  S.n_free = n_free;
  S.n_bound = n_bound;

  for (int q = 0; q < P.n_test; ++q) {
    const double* r = K + (size_t)P.test[q] * s.n;
    double sum = 0.0;
    for (int a = 0; a < l; ++a)
      if (alpha[a] != 0.0) sum += alpha[a] * y[a] * r[s.t[a]];
    dec[q] = sum - S.rho;
  }
}

// ---- the same solver with libsvm's shrinking (Solve(..., shrinking = 1)).
// The reference permutes the problem while it runs (swap_index,
// solver.cpp:47-57); here every array is indexed by *position*, t[k] is the
// Gram index and aset[k] the training-list index of the example at position
// k.  What decides the bits beyond the solver above:
//   - selection, the G update and rho run over the positions < active; ties
//     go to the last position (solver.cpp:368-443, :272-275, :561);
//   - Gb (G_bar) takes +- C_i Q_i[k] over all l positions when i enters or
//     leaves its upper bound, i before j, two roundings per entry (:279-306);
//   - reconstruct (:61-79): G[j] = Gb[j] + p[j], then + alpha_i Q_i[j] for the
//     free active positions i in ascending order, two roundings per term;
//   - shrink (:475-552): the two-pointer loop from both ends, and once, when
//     Gmax1 + Gmax2 <= 10 eps, reconstruct and the mirror loop from the tail
//     with the Gmax values from before;
//   - counter (:139-165) and the epilogue (:309-327) over the positions.
// Q_i[k] = (float)(y y K[t_i][t_k]) of the current occupants: the reference's
// row cache (qmatrix.cpp:37-60, Cache::swap_index) stores such values and
// changes none.
struct ShrinkSmo {
  const double* K;
  size_t n;
  int l, active;
  double Cp, Cn, eps;
  int64_t max_iter, iter = 0;
  std::vector<int32_t> t, aset;
  std::vector<signed char> y;
  std::vector<float> QD, Qi, Qj;
  std::vector<double> G, Gb, alpha;
  std::vector<char> st;
  bool unshrunk = false, stopped = false, pending = false;
  int32_t status = SK_SVM_CONVERGED;
  sk_svm_shrink_info info;

  double bound(int k) const { return y[k] > 0 ? Cp : Cn; }
  void set_status(int k) { st[k] = alpha[k] >= bound(k) ? kUpper : alpha[k] <= 0 ? kLower : kFree; }
  void row(int i, std::vector<float>& q, int len) const {
    const double* r = K + (size_t)t[i] * n;
    const int yi = y[i];
    for (int k = 0; k < len; ++k) q[k] = (float)(yi * y[k] * r[t[k]]);
  }
  void swap_positions(int a, int b) {
    std::swap(t[a], t[b]);
    std::swap(QD[a], QD[b]);
    std::swap(y[a], y[b]);
    std::swap(G[a], G[b]);
    std::swap(st[a], st[b]);
    std::swap(alpha[a], alpha[b]);
    std::swap(aset[a], aset[b]);
    std::swap(Gb[a], Gb[b]);
  }

  // the working pair over the active positions; false: optimal.  Leaves row i in Qi.
  bool pair(int& i, int& j) {
    double gmax = -kInf, gmax2 = -kInf, od_min = kInf;
    i = -1, j = -1;
    for (int k = 0; k < active; ++k) {
      if (y[k] > 0) {
        if (st[k] != kUpper && -G[k] >= gmax) gmax = -G[k], i = k;
      } else {
        if (st[k] != kLower && G[k] >= gmax) gmax = G[k], i = k;
      }
    }
    if (i >= 0) row(i, Qi, active);
    for (int k = 0; k < active; ++k) {
      double gd;
      float qf;
      if (y[k] > 0) {
        if (st[k] == kLower) continue;
        gd = gmax + G[k];
        if (G[k] >= gmax2) gmax2 = G[k];
        if (!(gd > 0)) continue;
        qf = Qi[i] + QD[k] - 2 * y[i] * Qi[k];  // float arithmetic
      } else {
        if (st[k] == kUpper) continue;
        gd = gmax - G[k];
        if (-G[k] >= gmax2) gmax2 = -G[k];
        if (!(gd > 0)) continue;
        qf = Qi[i] + QD[k] + 2 * y[i] * Qi[k];
      }
      const double qc = qf;
      const double od = qc > 0 ? -(gd * gd) / qc : -(gd * gd) / kTau;
      if (od <= od_min) od_min = od, j = k;
    }
    return !(gmax + gmax2 < eps);
  }

  // pair() with the iteration cap and the counters: once max_iter updates
  // have run and a further pair was found (or none can be), this and every
  // later selection report optimal, so the loop below reconstructs the
  // gradient, restores the active set and ends
  bool select(int& i, int& j) {
    if (stopped) return false;
    const bool after_reconstruction = pending;
    pending = false;
    if (!pair(i, j)) {
      if (active < l) ++info.reconstructions, pending = true;
      return false;
    }
    if (i < 0 || j < 0) {
      status = SK_SVM_NO_PAIR, stopped = true;
      return false;
    }
    if (iter == max_iter) {
      status = SK_SVM_NOT_CONVERGED, stopped = true;
      return false;
    }
    if (after_reconstruction) ++info.resumed;
    return true;
  }

  void reconstruct() {
    if (active == l) return;
    for (int k = active; k < l; ++k) G[k] = Gb[k] + -1.0;
    for (int i = 0; i < active; ++i)
      if (st[i] == kFree) {
        row(i, Qi, l);
        const double a = alpha[i];
        for (int k = active; k < l; ++k) G[k] += a * Qi[k];
      }
  }

  bool shrinkable(int k, double g1, double g2) const {
    if (st[k] == kUpper) return y[k] > 0 ? -G[k] > g1 : -G[k] > g2;
    if (st[k] == kLower) return y[k] > 0 ? G[k] > g2 : G[k] > g1;
    return false;
  }

  void shrink() {
    ++info.shrink_calls;
    const int before = active;
    double g1 = -kInf, g2 = -kInf;  // max of -y G over I_up, of y G over I_low
    for (int k = 0; k < active; ++k) {
      if (y[k] > 0) {
        if (st[k] != kUpper && -G[k] >= g1) g1 = -G[k];
        if (st[k] != kLower && G[k] >= g2) g2 = G[k];
      } else {
        if (st[k] != kUpper && -G[k] >= g2) g2 = -G[k];
        if (st[k] != kLower && G[k] >= g1) g1 = G[k];
      }
    }
    for (int k = 0; k < active; ++k)
      if (shrinkable(k, g1, g2))
        for (--active; active > k; --active)
          if (!shrinkable(active, g1, g2)) {
            swap_positions(k, active);
            break;
          }
    if (!unshrunk && !(g1 + g2 > eps * 10)) {
      unshrunk = true;
      info.unshrunk = 1;
      reconstruct();
      for (int k = l - 1; k >= active; --k)
        if (!shrinkable(k, g1, g2)) {
          for (; active < k; ++active)
            if (shrinkable(active, g1, g2)) {
              swap_positions(k, active);
              break;
            }
          ++active;
        }
      if (active > before) info.regrown = 1;
    }
    if (active < before) ++info.shrunk_calls;
    info.min_active = std::min(info.min_active, active);
  }
};

void solve_one_shrink(const double* K, int32_t n, const double* labels, const sk_svm_problem& P, double* alpha_out,
                      double* dec, sk_svm_solution& S, sk_svm_shrink_info& info) {
  ShrinkSmo s;
  s.K = K;
  s.n = (size_t)n;
  const int l = s.l = s.active = P.n_train;
  s.Cp = P.Cp, s.Cn = P.Cn, s.eps = P.eps, s.max_iter = P.max_iter;
  s.info = sk_svm_shrink_info{0, 0, l, 0, 0, 0, 0};
  s.t.assign(P.train, P.train + l);
  s.aset.resize(l);
  s.y.resize(l);
  s.QD.resize(l);
  s.Qi.resize(l);
  s.Qj.resize(l);
  s.G.assign(l, -1.0);
  s.Gb.assign(l, 0.0);
  s.alpha.assign(l, 0.0);
  s.st.assign(l, kLower);
  for (int k = 0; k < l; ++k) {
    s.aset[k] = k;
    s.y[k] = labels[s.t[k]] > 0 ? +1 : -1;
    s.QD[k] = (float)K[(size_t)s.t[k] * s.n + s.t[k]];
  }
  std::vector<double>&G = s.G, &Gb = s.Gb, &alpha = s.alpha;
  const std::vector<float>&Qi = s.Qi, &Qj = s.Qj;

  const int period = std::min(l, 1000);
  int counter = period + 1;
  for (;;) {
    if (--counter == 0) {
      counter = period;
      s.shrink();
    }
    int i, j;
    if (!s.select(i, j)) {
      s.reconstruct();
      s.active = l;
      if (!s.select(i, j)) break;
      counter = 1;  // shrink at the next iteration
    }
    ++s.iter;
    const int active = s.active;
    s.row(j, s.Qj, active);  // row i is in Qi since the selection
    const double Ci = s.bound(i), Cj = s.bound(j);
    const double ai0 = alpha[i], aj0 = alpha[j];
    update_pair(s.y[i] != s.y[j], Qi[i], Qj[j], Qi[j], G[i], G[j], Ci, Cj, alpha[i], alpha[j]);
    const double dai = alpha[i] - ai0, daj = alpha[j] - aj0;
    for (int k = 0; k < active; ++k) G[k] += Qi[k] * dai + Qj[k] * daj;
    const bool ui = s.st[i] == kUpper, uj = s.st[j] == kUpper;
    s.set_status(i);
    s.set_status(j);
    if (ui != (s.st[i] == kUpper)) {
      s.row(i, s.Qi, l);
      if (ui)
        for (int k = 0; k < l; ++k) Gb[k] -= Ci * Qi[k];
      else
        for (int k = 0; k < l; ++k) Gb[k] += Ci * Qi[k];
    }
    if (uj != (s.st[j] == kUpper)) {
      s.row(j, s.Qj, l);
      if (uj)
        for (int k = 0; k < l; ++k) Gb[k] -= Cj * Qj[k];
      else
        for (int k = 0; k < l; ++k) Gb[k] += Cj * Qj[k];
    }
  }

  // rho, obj: in position order; the alphas go back to training order
  int n_free = 0, n_bound = 0;
  double ub = kInf, lb = -kInf, sum_free = 0;
  for (int k = 0; k < l; ++k) {
    const double yg = s.y[k] * G[k];
    if (s.st[k] == kUpper) {
      ++n_bound;
      if (s.y[k] < 0) ub = std::min(ub, yg);
      else lb = std::max(lb, yg);
    } else if (s.st[k] == kLower) {
      if (s.y[k] > 0) ub = std::min(ub, yg);
      else lb = std::max(lb, yg);
    } else {
      ++n_free;
      sum_free += yg;
    }
  }
  S.rho = n_free > 0 ? sum_free / n_free : (ub + lb) / 2;
  double v = 0;
  for (int k = 0; k < l; ++k) v += alpha[k] * (G[k] + -1.0);
  S.obj = v / 2;
  S.iterations = s.iter;
  S.status = s.status;
  S.n_free = n_free;
  S.n_bound = n_bound;
  info = s.info;
  for (int k = 0; k < l; ++k) alpha_out[s.aset[k]] = alpha[k];

  for (int q = 0; q < P.n_test; ++q) {
    const double* r = K + (size_t)P.test[q] * s.n;
    double sum = 0.0;
    for (int a = 0; a < l; ++a)
      if (alpha_out[a] != 0.0) sum += alpha_out[a] * (labels[P.train[a]] > 0 ? 1 : -1) * r[P.train[a]];
    dec[q] = sum - S.rho;
  }
}

// ---- the general Solve and Solver_NU, without shrinking: what nu-SVC,
// one-class, epsilon-SVR and nu-SVR run (sk_svm_solve_batch_host).
//   Solver::Solve            solver.cpp:81-349, the start :113-135 with a
//                            general p and alpha
//   Solver_NU                select_working_set solver.cpp:595-705,
//                            calculate_rho :799-848
//   SVC_Q / ONE_CLASS_Q / SVR_Q  qmatrix.cpp:339-475: over positions all three
//                            are Q_i[k] = y_i y_k (float)K[t_i][t_k]
// A position k is (Gram index t[k], y[k]); SVR has 2 l of them over l examples.
struct GenSmo {
  const double* K;
  size_t n;
  int l;  // positions
  double C, eps;
  int64_t max_iter;
  std::vector<int32_t> t;
  std::vector<signed char> y;
  std::vector<float> QD, Qp, Qn, Qj;
  std::vector<double> G, p, alpha;
  std::vector<char> st;
  // results
  double rho = 0, obj = 0, r = 0;
  int64_t iter = 0;
  int32_t status = SK_SVM_CONVERGED, n_free = 0, n_bound = 0;

  void set_status(int k) { st[k] = alpha[k] >= C ? kUpper : alpha[k] <= 0 ? kLower : kFree; }
  void row(int i, std::vector<float>& q) const {
    const double* r_ = K + (size_t)t[i] * n;
    const int yi = y[i];
    for (int k = 0; k < l; ++k) q[k] = (float)(yi * y[k]) * (float)r_[t[k]];
  }

  void start() {
    QD.resize(l), Qp.resize(l), Qn.resize(l), Qj.resize(l), st.resize(l);
    G = p;
    for (int k = 0; k < l; ++k) {
      QD[k] = (float)K[(size_t)t[k] * n + t[k]];
      set_status(k);
    }
    for (int i = 0; i < l; ++i)
      if (st[i] != kLower) {
        row(i, Qp);
        const double a = alpha[i];
        for (int j = 0; j < l; ++j) G[j] += a * Qp[j];
      }
  }

  void update(int i, int j, const std::vector<float>& Qi) {
    row(j, Qj);
    const double ai0 = alpha[i], aj0 = alpha[j];
    update_pair(y[i] != y[j], Qi[i], Qj[j], Qi[j], G[i], G[j], C, C, alpha[i], alpha[j]);
    const double dai = alpha[i] - ai0, daj = alpha[j] - aj0;
    for (int k = 0; k < l; ++k) G[k] += Qi[k] * dai + Qj[k] * daj;
    set_status(i);
    set_status(j);
  }

  // Solver::select_working_set and Solver::calculate_rho
  void solve_plain() {
    std::vector<float>& Qi = Qp;
    for (;;) {
      double gmax = -kInf, gmax2 = -kInf, od_min = kInf;
      int i = -1, j = -1;
      for (int k = 0; k < l; ++k) {
        if (y[k] > 0) {
          if (st[k] != kUpper && -G[k] >= gmax) gmax = -G[k], i = k;
        } else {
          if (st[k] != kLower && G[k] >= gmax) gmax = G[k], i = k;
        }
      }
      if (i >= 0) row(i, Qi);
      for (int k = 0; k < l; ++k) {
        double gd;
        float qf;
        if (y[k] > 0) {
          if (st[k] == kLower) continue;
          gd = gmax + G[k];
          if (G[k] >= gmax2) gmax2 = G[k];
          if (!(gd > 0)) continue;
          qf = Qi[i] + QD[k] - 2 * y[i] * Qi[k];  // float arithmetic
        } else {
          if (st[k] == kUpper) continue;
          gd = gmax - G[k];
          if (-G[k] >= gmax2) gmax2 = -G[k];
          if (!(gd > 0)) continue;
          qf = Qi[i] + QD[k] + 2 * y[i] * Qi[k];
        }
        const double qc = qf;
        const double od = qc > 0 ? -(gd * gd) / qc : -(gd * gd) / kTau;
        if (od <= od_min) od_min = od, j = k;
      }
      if (gmax + gmax2 < eps) break;
      if (i < 0 || j < 0) {
        status = SK_SVM_NO_PAIR;
        break;
      }
      if (iter == max_iter) {
        status = SK_SVM_NOT_CONVERGED;
        break;
      }
      ++iter;
      update(i, j, Qi);
    }
    double ub = kInf, lb = -kInf, sum_free = 0;
    for (int k = 0; k < l; ++k) {
      const double yg = y[k] * G[k];
      if (st[k] == kUpper) {
        ++n_bound;
        if (y[k] < 0) ub = std::min(ub, yg);
        else lb = std::max(lb, yg);
      } else if (st[k] == kLower) {
        if (y[k] > 0) ub = std::min(ub, yg);
        else lb = std::max(lb, yg);
      } else {
        ++n_free;
        sum_free += yg;
      }
    }
    rho = n_free > 0 ? sum_free / n_free : (ub + lb) / 2;
    r = 0;
  }

  // Solver_NU::select_working_set and Solver_NU::calculate_rho
  void solve_nu() {
    for (;;) {
      double gmaxp = -kInf, gmaxp2 = -kInf, gmaxn = -kInf, gmaxn2 = -kInf, od_min = kInf;
      int ip = -1, in = -1, j = -1;
      for (int k = 0; k < l; ++k) {
        if (y[k] > 0) {
          if (st[k] != kUpper && -G[k] >= gmaxp) gmaxp = -G[k], ip = k;
        } else {
          if (st[k] != kLower && G[k] >= gmaxn) gmaxn = G[k], in = k;
        }
      }
      if (ip >= 0) row(ip, Qp);
      if (in >= 0) row(in, Qn);
      for (int k = 0; k < l; ++k) {
        double gd;
        float qf;
        if (y[k] > 0) {
          if (st[k] == kLower) continue;
          gd = gmaxp + G[k];
          if (G[k] >= gmaxp2) gmaxp2 = G[k];
          if (!(gd > 0)) continue;
          qf = Qp[ip] + QD[k] - 2 * Qp[k];  // float arithmetic; gd > 0 implies ip >= 0
        } else {
          if (st[k] == kUpper) continue;
          gd = gmaxn - G[k];
          if (-G[k] >= gmaxn2) gmaxn2 = -G[k];
          if (!(gd > 0)) continue;
          qf = Qn[in] + QD[k] - 2 * Qn[k];
        }
        const double qc = qf;
        const double od = qc > 0 ? -(gd * gd) / qc : -(gd * gd) / kTau;
        if (od <= od_min) od_min = od, j = k;
      }
      if (std::max(gmaxp + gmaxp2, gmaxn + gmaxn2) < eps) break;
      const int i = j < 0 ? -1 : y[j] > 0 ? ip : in;
      if (i < 0 || j < 0) {  // the reference reads y[-1] here
        status = SK_SVM_NO_PAIR;
        break;
      }
      if (iter == max_iter) {
        status = SK_SVM_NOT_CONVERGED;
        break;
      }
      ++iter;
      update(i, j, y[j] > 0 ? Qp : Qn);
    }
    int nf1 = 0, nf2 = 0;
    double ub1 = kInf, ub2 = kInf, lb1 = -kInf, lb2 = -kInf, sum1 = 0, sum2 = 0;
    for (int k = 0; k < l; ++k) {
      if (st[k] == kUpper) ++n_bound;
      if (y[k] > 0) {
        if (st[k] == kUpper) lb1 = std::max(lb1, G[k]);
        else if (st[k] == kLower) ub1 = std::min(ub1, G[k]);
        else ++nf1, sum1 += G[k];
      } else {
        if (st[k] == kUpper) lb2 = std::max(lb2, G[k]);
        else if (st[k] == kLower) ub2 = std::min(ub2, G[k]);
        else ++nf2, sum2 += G[k];
      }
    }
    const double r1 = nf1 > 0 ? sum1 / nf1 : (ub1 + lb1) / 2;
    const double r2 = nf2 > 0 ? sum2 / nf2 : (ub2 + lb2) / 2;
    n_free = nf1 + nf2;
    r = (r1 + r2) / 2;
    rho = (r1 - r2) / 2;
  }

  void solve(bool nu) {
    start();
    if (nu) solve_nu();
    else solve_plain();
    double v = 0;
    for (int k = 0; k < l; ++k) v += alpha[k] * (G[k] + p[k]);
    obj = v / 2;
  }
};

// One task of sk_svm_solve_batch_host: what svm_train_one leaves (svm.cpp:245-300)
void solve_task(const double* K, int32_t n, const double* targets, const sk_svm_task& T, double* coef, double* dec,
                sk_svm_task_solution& S) {
  const int l = T.n_train;
  if (T.svm_type == SK_SVM_C_SVC) {
    sk_svm_problem P = {T.train, T.n_train, nullptr, 0, T.C, T.C, T.eps, T.max_iter};
    sk_svm_solution s;
    solve_one(K, n, targets, P, coef, nullptr, s);
    for (int k = 0; k < l; ++k) coef[k] *= targets[T.train[k]] > 0 ? 1 : -1;
    S.rho = s.rho, S.obj = s.obj, S.iterations = s.iterations, S.status = s.status, S.n_free = s.n_free,
    S.n_bound = s.n_bound, S.r = 0;
  } else {
    GenSmo g;
    g.K = K, g.n = (size_t)n, g.eps = T.eps, g.max_iter = T.max_iter;
    std::vector<int32_t> ty;
    g.l = sk::svm_task_positions(targets, T, ty, g.p, g.alpha, &g.C);
    g.t.resize(g.l), g.y.resize(g.l);
    for (int k = 0; k < g.l; ++k) g.t[k] = ty[k] >> 1, g.y[k] = (ty[k] & 1) ? +1 : -1;
    g.solve(sk::svm_type_is_nu(T.svm_type));
    S.rho = g.rho, S.obj = g.obj, S.r = g.r, S.iterations = g.iter, S.status = g.status, S.n_free = g.n_free,
    S.n_bound = g.n_bound;
    if (T.svm_type == SK_SVM_NU_SVC) {
      const double r = g.r;
      for (int k = 0; k < l; ++k) coef[k] = g.alpha[k] * (g.y[k] / r);
      S.rho /= r;
      S.obj /= (r * r);
    } else if (T.svm_type == SK_SVM_ONE_CLASS) {
      for (int k = 0; k < l; ++k) coef[k] = g.alpha[k];
    } else {
      for (int k = 0; k < l; ++k) coef[k] = g.alpha[k] - g.alpha[k + l];
    }
  }
  for (int q = 0; q < T.n_test; ++q) {
    const double* r = K + (size_t)T.test[q] * (size_t)n;
    double sum = 0.0;
    for (int a = 0; a < l; ++a)
      if (coef[a] != 0.0) sum += coef[a] * r[T.train[a]];
    dec[q] = sum - S.rho;
  }
}

// A two-class model in svm_save_model's text (svm.cpp:1201-1286) from signed
// coefficients (alpha y for C-SVC, alpha y / r for nu-SVC)
int write_classifier(const char* path, const char* type_name, const double* labels, int32_t n, const int32_t* train,
                     int32_t n_train, const double* coef, double rho) {
  // svm_group_classes: classes by first appearance of the (int) label
  int lab[2] = {0, 0}, ncls = 0;
  bool pos[2] = {false, false};
  std::vector<signed char> cls(n_train);
  for (int k = 0; k < n_train; ++k) {
    if (train[k] < 0 || train[k] >= n) return SK_ERR_INVALID;
    const double v = labels[train[k]];
    if (!(std::fabs(v) < 2147483648.0)) return SK_ERR_INVALID;
    const int il = (int)v;
    int c = 0;
    while (c < ncls && lab[c] != il) ++c;
    if (c == ncls) {
      if (ncls == 2) return SK_ERR_INVALID;
      lab[ncls] = il;
      pos[ncls++] = v > 0;
    } else if (pos[c] != (v > 0)) {
      return SK_ERR_INVALID;  // one (int) label on both sides of the solver's y
    }
    cls[k] = (signed char)c;
  }
  if (ncls != 2 || pos[0] == pos[1]) return SK_ERR_INVALID;
  // libsvm's +1 is its first class: the solver's y = +1 is label > 0
  const double sgn = pos[0] ? 1.0 : -1.0;
  int nsv[2] = {0, 0};
  for (int k = 0; k < n_train; ++k)
    if (coef[k] != 0.0) ++nsv[cls[k]];
  FILE* f = std::fopen(path, "w");
  if (!f) return SK_ERR_INVALID;
  std::fprintf(f, "svm_type %s\nkernel_type precomputed\nnr_class 2\ntotal_sv %d\n", type_name, nsv[0] + nsv[1]);
  std::fprintf(f, "rho %g\nlabel %d %d\nnr_sv %d %d\nSV\n", sgn * rho, lab[0], lab[1], nsv[0], nsv[1]);
  for (int c = 0; c < 2; ++c)
    for (int k = 0; k < n_train; ++k)
      if (cls[k] == c && coef[k] != 0.0) std::fprintf(f, "%.16g 0:%d \n", sgn * coef[k], train[k] + 1);
  const bool bad = std::ferror(f) != 0;
  return (std::fclose(f) != 0 || bad) ? SK_ERR_INVALID : SK_OK;
}

// fn(p) for p in [0, count) on n_threads threads (0 = hardware concurrency),
// the calling thread among them; SK_ERR_ALLOC when one ran out of memory
template <class F>
int run_pool(int count, int n_threads, F fn) {
  int nt = n_threads ? n_threads : (int)std::max(1u, std::thread::hardware_concurrency());
  nt = std::max(1, std::min(nt, count));
  std::atomic<int> cursor{0};
  std::atomic<bool> oom{false};
  auto work = [&] {
    for (int p; (p = cursor.fetch_add(1)) < count;) {
      try {
        fn(p);
      } catch (const std::bad_alloc&) {
        oom = true;
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t) {
    try {
      th.emplace_back(work);
    } catch (const std::system_error&) {
      break;  // the calling thread's share drains the cursor
    }
  }
  work();
  for (auto& x : th) x.join();
  return oom ? SK_ERR_ALLOC : SK_OK;
}

}  // namespace

namespace sk {

int svm_task_positions(const double* targets, const sk_svm_task& T, std::vector<int32_t>& ty, std::vector<double>& p,
                       std::vector<double>& alpha0, double* C) {
  const int l = T.n_train;
  const size_t at = ty.size();
  const bool svr = svm_type_is_svr(T.svm_type);
  const int L = svr ? 2 * l : l;
  ty.resize(at + L), p.resize(at + L), alpha0.resize(at + L);
  int32_t* y_ = ty.data() + at;
  double* p_ = p.data() + at;
  double* a_ = alpha0.data() + at;
  if (T.svm_type == SK_SVM_NU_SVC) {
    const double nu = T.nu;
    double sum_pos = nu * l / 2, sum_neg = nu * l / 2;
    for (int k = 0; k < l; ++k) {
      const bool pos = targets[T.train[k]] > 0;
      double& sum = pos ? sum_pos : sum_neg;
      a_[k] = std::min(1.0, sum);
      sum -= a_[k];
      p_[k] = 0;
      y_[k] = (T.train[k] << 1) | (pos ? 1 : 0);
    }
    *C = 1.0;
  } else if (T.svm_type == SK_SVM_ONE_CLASS) {
    const int m = (int)(T.nu * l);  // alphas at the upper bound
    for (int k = 0; k < l; ++k) {
      a_[k] = k < m ? 1 : 0;
      p_[k] = 0;
      y_[k] = (T.train[k] << 1) | 1;
    }
    if (m < l) a_[m] = T.nu * l - m;
    *C = 1.0;
  } else if (T.svm_type == SK_SVM_EPSILON_SVR) {
    for (int k = 0; k < l; ++k) {
      const double v = targets[T.train[k]];
      a_[k] = a_[k + l] = 0;
      p_[k] = T.p - v;
      p_[k + l] = T.p + v;
      y_[k] = (T.train[k] << 1) | 1;
      y_[k + l] = T.train[k] << 1;
    }
    *C = T.C;
  } else {  // SK_SVM_NU_SVR
    double sum = T.C * T.nu * l / 2;
    for (int k = 0; k < l; ++k) {
      const double v = targets[T.train[k]];
      a_[k] = a_[k + l] = std::min(sum, T.C);
      sum -= a_[k];
      p_[k] = -v;
      p_[k + l] = v;
      y_[k] = (T.train[k] << 1) | 1;
      y_[k + l] = T.train[k] << 1;
    }
    *C = T.C;
  }
  return L;
}

int svm_check_tasks(const double* gram, int32_t n, const double* targets, const sk_svm_task* tasks, int32_t n_tasks,
                    const double* coef_out, const double* dec_out, const sk_svm_task_solution* solutions,
                    bool on_gpu, int64_t* sum_train, int64_t* sum_test, std::string& err) {
  auto bad = [&](int p, const char* what) {
    err = "sk_svm_solve_batch: task " + std::to_string(p) + ": " + what;
    return (int)SK_ERR_INVALID;
  };
  if (!gram || n < 1 || n_tasks < 0 || (n_tasks && !tasks) || !coef_out || (n_tasks && !solutions)) {
    err = "sk_svm_solve_batch: null or empty argument";
    return SK_ERR_INVALID;
  }
  int64_t st = 0, ss = 0;
  for (int p = 0; p < n_tasks; ++p) {
    const sk_svm_task& T = tasks[p];
    const int ty = T.svm_type;
    if (ty < SK_SVM_C_SVC || ty > SK_SVM_NU_SVR) return bad(p, "unknown svm type");
    if (ty != SK_SVM_ONE_CLASS && !targets) return bad(p, "targets is null");
    if (T.n_train < 2 || !T.train) return bad(p, "n_train < 2");
    if (T.n_test < 0 || (T.n_test && !T.test)) return bad(p, "test list");
    if (!(T.eps > 0)) return bad(p, "eps <= 0");
    if (T.max_iter < 1) return bad(p, "max_iter < 1");
    if ((ty == SK_SVM_C_SVC || svm_type_is_svr(ty)) && !(T.C > 0)) return bad(p, "C <= 0");
    if ((ty == SK_SVM_NU_SVC || ty == SK_SVM_ONE_CLASS || ty == SK_SVM_NU_SVR) && !(T.nu > 0 && T.nu <= 1))
      return bad(p, "nu <= 0 or nu > 1");
    if (ty == SK_SVM_EPSILON_SVR && !(T.p >= 0)) return bad(p, "p < 0");
    int64_t np = 0, nn = 0;
    for (int k = 0; k < T.n_train; ++k) {
      const int32_t t = T.train[k];
      if (t < 0 || t >= n) return bad(p, "training index outside [0, n)");
      if (svm_type_is_svr(ty)) {
        if (!std::isfinite(targets[t])) return bad(p, "a target that is not finite");
      } else if (ty != SK_SVM_ONE_CLASS) {
        ++(targets[t] > 0 ? np : nn);
      }
    }
    for (int k = 0; k < T.n_test; ++k)
      if (T.test[k] < 0 || T.test[k] >= n) return bad(p, "test index outside [0, n)");
    if (ty == SK_SVM_C_SVC || ty == SK_SVM_NU_SVC) {
      if (!np || !nn) return bad(p, "training list with one class only");
      if (ty == SK_SVM_NU_SVC && T.nu * (double)(np + nn) / 2 > (double)std::min(np, nn))
        return bad(p, "specified nu is infeasible");
    }
    st += T.n_train;
    ss += T.n_test;
  }
  if (ss && !dec_out) {
    err = "sk_svm_solve_batch: dec_out is null";
    return SK_ERR_INVALID;
  }
  if (on_gpu)
    for (int p = 0; p < n_tasks; ++p)
      if (tasks[p].n_train > svm_type_max_train(tasks[p].svm_type)) {
        err = "sk_svm_solve_batch: task " + std::to_string(p) + ": n_train " + std::to_string(tasks[p].n_train) +
              " over the GPU solver's " + std::to_string(svm_type_max_train(tasks[p].svm_type)) + " for its type";
        return SK_ERR_UNSUPPORTED;
      }
  *sum_train = st;
  *sum_test = ss;
  return SK_OK;
}

int svm_check_batch(const double* gram, int32_t n, const double* labels, const sk_svm_problem* problems,
                    int32_t n_problems, const double* alpha_out, const double* dec_out,
                    const sk_svm_solution* solutions, int32_t max_train, int64_t* sum_train,
                    int64_t* sum_test, std::string& err) {
  auto bad = [&](int p, const char* what) {
    err = "sk_svm_train_batch: problem " + std::to_string(p) + ": " + what;
    return (int)SK_ERR_INVALID;
  };
  if (!gram || !labels || n < 1 || n_problems < 0 || (n_problems && !problems) || !alpha_out ||
      (n_problems && !solutions)) {
    err = "sk_svm_train_batch: null or empty argument";
    return SK_ERR_INVALID;
  }
  int64_t st = 0, ss = 0;
  for (int p = 0; p < n_problems; ++p) {
    const sk_svm_problem& P = problems[p];
    if (P.n_train < 2 || !P.train) return bad(p, "n_train < 2");
    if (P.n_test < 0 || (P.n_test && !P.test)) return bad(p, "test list");
    if (!(P.eps > 0)) return bad(p, "eps <= 0");
    if (!(P.Cp > 0) || !(P.Cn > 0)) return bad(p, "C <= 0");
    if (P.max_iter < 1) return bad(p, "max_iter < 1");
    bool pos = false, neg = false;
    for (int k = 0; k < P.n_train; ++k) {
      const int32_t t = P.train[k];
      if (t < 0 || t >= n) return bad(p, "training index outside [0, n)");
      (labels[t] > 0 ? pos : neg) = true;
    }
    for (int k = 0; k < P.n_test; ++k)
      if (P.test[k] < 0 || P.test[k] >= n) return bad(p, "test index outside [0, n)");
    if (!pos || !neg) return bad(p, "training list with one class only");
    st += P.n_train;
    ss += P.n_test;
  }
  if (ss && !dec_out) {
    err = "sk_svm_train_batch: dec_out is null";
    return SK_ERR_INVALID;
  }
  if (max_train > 0)
    for (int p = 0; p < n_problems; ++p)
      if (problems[p].n_train > max_train) {
        err = "sk_svm_train_batch: problem " + std::to_string(p) + ": n_train " +
              std::to_string(problems[p].n_train) + " over the GPU solver's " + std::to_string(max_train);
        return SK_ERR_UNSUPPORTED;
      }
  *sum_train = st;
  *sum_test = ss;
  return SK_OK;
}

}  // namespace sk

extern "C" {

int sk_svm_train_batch_host_ex(const double* gram, int32_t n, const double* labels, const sk_svm_problem* problems,
                               int32_t n_problems, int32_t n_threads, int32_t shrinking, double* alpha_out,
                               double* dec_out, sk_svm_solution* solutions, sk_svm_shrink_info* info) {
  try {
    std::string err;
    int64_t st = 0, ss = 0;
    const int rc = sk::svm_check_batch(gram, n, labels, problems, n_problems, alpha_out, dec_out, solutions, 0,
                                       &st, &ss, err);
    if (rc) return rc;
    if (n_threads < 0) return SK_ERR_INVALID;
    std::vector<int64_t> aoff(n_problems + 1, 0), doff(n_problems + 1, 0);
    for (int p = 0; p < n_problems; ++p) {
      aoff[p + 1] = aoff[p] + problems[p].n_train;
      doff[p + 1] = doff[p] + problems[p].n_test;
    }
    return run_pool(n_problems, n_threads, [&](int p) {
      double* dec = dec_out ? dec_out + doff[p] : nullptr;
      sk_svm_shrink_info si = {0, 0, problems[p].n_train, 0, 0, 0, 0};
      if (shrinking)
        solve_one_shrink(gram, n, labels, problems[p], alpha_out + aoff[p], dec, solutions[p], si);
      else
        solve_one(gram, n, labels, problems[p], alpha_out + aoff[p], dec, solutions[p]);
      if (info) info[p] = si;
    });
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
}

int sk_svm_train_batch_host(const double* gram, int32_t n, const double* labels, const sk_svm_problem* problems,
                            int32_t n_problems, int32_t n_threads, double* alpha_out, double* dec_out,
                            sk_svm_solution* solutions) {
  return sk_svm_train_batch_host_ex(gram, n, labels, problems, n_problems, n_threads, 0, alpha_out, dec_out,
                                    solutions, nullptr);
}

int sk_svm_train_shape(int32_t* bounds, int32_t* n_classes, int32_t* max_train) {
  if (bounds)
    for (int c = 0; c < sk::kSvmClasses; ++c) bounds[c] = sk::kSvmThreads[c] * sk::kSvmElems;
  if (n_classes) *n_classes = sk::kSvmClasses;
  if (max_train) *max_train = sk::kSvmMaxTrain;
  return SK_OK;
}

int sk_svm_solve_batch_host(const double* gram, int32_t n, const double* targets, const sk_svm_task* tasks,
                            int32_t n_tasks, int32_t n_threads, double* coef_out, double* dec_out,
                            sk_svm_task_solution* solutions) {
  try {
    std::string err;
    int64_t st = 0, ss = 0;
    const int rc =
        sk::svm_check_tasks(gram, n, targets, tasks, n_tasks, coef_out, dec_out, solutions, false, &st, &ss, err);
    if (rc) return rc;
    if (n_threads < 0) return SK_ERR_INVALID;
    std::vector<int64_t> aoff(n_tasks + 1, 0), doff(n_tasks + 1, 0);
    for (int p = 0; p < n_tasks; ++p) {
      aoff[p + 1] = aoff[p] + tasks[p].n_train;
      doff[p + 1] = doff[p] + tasks[p].n_test;
    }
    return run_pool(n_tasks, n_threads, [&](int p) {
      solve_task(gram, n, targets, tasks[p], coef_out + aoff[p], dec_out ? dec_out + doff[p] : nullptr, solutions[p]);
    });
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
}

int sk_svm_solve_shape(int32_t* max_train) {
  if (max_train)
    for (int t = SK_SVM_C_SVC; t <= SK_SVM_NU_SVR; ++t) max_train[t] = sk::svm_type_max_train(t);
  return SK_OK;
}

int sk_svm_model_write(const char* path, const double* labels, int32_t n, const int32_t* train, int32_t n_train,
                       const double* alpha, double rho) {
  if (!path || !labels || !train || !alpha || n_train < 2) return SK_ERR_INVALID;
  try {
    std::vector<double> coef(n_train);
    for (int k = 0; k < n_train; ++k) {
      if (train[k] < 0 || train[k] >= n) return SK_ERR_INVALID;
      coef[k] = alpha[k] * (labels[train[k]] > 0 ? 1 : -1);
    }
    return write_classifier(path, "c_svc", labels, n, train, n_train, coef.data(), rho);
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
}

int sk_svm_model_write_ex(const char* path, int32_t svm_type, const double* targets, int32_t n, const int32_t* train,
                          int32_t n_train, const double* coef, double rho) {
  static const char* const names[] = {"c_svc", "nu_svc", "one_class", "epsilon_svr", "nu_svr"};
  if (!path || !train || !coef || n_train < 2 || svm_type < SK_SVM_C_SVC || svm_type > SK_SVM_NU_SVR)
    return SK_ERR_INVALID;
  try {
    if (svm_type == SK_SVM_C_SVC || svm_type == SK_SVM_NU_SVC)
      return targets ? write_classifier(path, names[svm_type], targets, n, train, n_train, coef, rho)
                     : (int)SK_ERR_INVALID;
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
  // one-class and regression (svm_train, svm.cpp:677-717): nr_class 2, no
  // label and nr_sv lines, the examples with fabs(coef) > 0 in list order
  int total = 0;
  for (int k = 0; k < n_train; ++k) {
    if (train[k] < 0 || train[k] >= n) return SK_ERR_INVALID;
    if (std::fabs(coef[k]) > 0) ++total;
  }
  FILE* f = std::fopen(path, "w");
  if (!f) return SK_ERR_INVALID;
  std::fprintf(f, "svm_type %s\nkernel_type precomputed\nnr_class 2\ntotal_sv %d\nrho %g\nSV\n", names[svm_type],
               total, rho);
  for (int k = 0; k < n_train; ++k)
    if (std::fabs(coef[k]) > 0) std::fprintf(f, "%.16g 0:%d \n", coef[k], train[k] + 1);
  const bool bad = std::ferror(f) != 0;
  return (std::fclose(f) != 0 || bad) ? SK_ERR_INVALID : SK_OK;
}

}  // extern "C"
