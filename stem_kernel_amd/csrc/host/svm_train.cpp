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
// SVM training on a precomputed Gram: the reference's SMO solver, restated
// from the published algorithm (Fan, Chen and Lin, JMLR 6 (2005), working-set
// selection 3).  As in libsvm there is one Solver, and Solver_NU is the same
// with another selection and another rho (the template parameter NU below):
//   Solver::Solve            libsvm/solver.cpp:81-349   (start :113-135,
//                            counter :139-165, the two-variable update
//                            :180-265, G update :272-275, G_bar :279-306,
//                            obj :314-321)
//   select_working_set       solver.cpp:352-451
//   calculate_rho            solver.cpp:554-592
//   swap_index               solver.cpp:47-57
//   reconstruct_gradient     solver.cpp:61-79
//   do_shrinking             solver.cpp:475-552
//   Solver_NU                select_working_set solver.cpp:595-705,
//                            calculate_rho :799-848
//   update_alpha_status      libsvm/solver.h:67-74
//   SVC_Q / ONE_CLASS_Q / SVR_Q  libsvm/qmatrix.cpp:339-475 (QD, get_Q: float)
//   kernel_precomputed       qmatrix.cpp:331-336
//   svm_train_one            libsvm/svm.cpp:245-300, which sets a problem up
//                            through solve_c_svc :38-71 (p = -1, alpha = 0, y),
//                            solve_nu_svc :73-126, solve_one_class :128-158,
//                            solve_epsilon_svr :160-196, solve_nu_svr :198-234
//   svm_check_parameter      svm.cpp:1499-1615
//   svm_train / svm_predict  optimizer/gradient.cpp:208-246, :248-278
//   svm_save_model           svm.cpp:1201-1286, svm_group_classes :611-666;
//                            the one-class / regression model svm.cpp:677-717
// The solver works on positions: position k is (Gram index t[k], y[k]) with a
// linear term p[k] and an upper bound C[k]; SVR has 2 l of them over l
// examples (sk::svm_task_positions builds them for all five types).  Shrinking
// is built for C-SVC: Solver_NU::do_shrinking is not restated, and the other
// four formulations are solved without.
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

// Solver::Solve over positions.  The reference permutes the problem while it
// shrinks (swap_index); here every array is indexed by *position*, and aset[k]
// is the position the occupant of k started at.  What decides the bits:
//   - Q_i[k] = (float)(y_i y_k K[t_i][t_k]) of the current occupants: the
//     reference's row cache (qmatrix.cpp:37-60, Cache::swap_index) stores such
//     values and changes none;
//   - selection, the G update and the counter run over the positions < active
//     (all l without shrinking); ties go to the last position (solver.cpp:
//     368-443, :272-275);
//   - Gb (G_bar) takes +- C_i Q_i[k] over all l positions when i enters or
//     leaves its upper bound, i before j, two roundings per entry (:279-306);
//     kept with shrinking only, nothing else reads it;
//   - reconstruct (:61-79): G[j] = Gb[j] + p[j], then + alpha_i Q_i[j] for the
//     free active positions i in ascending order, two roundings per term;
//   - shrink (:475-552): the two-pointer loop from both ends, and once, when
//     Gmax1 + Gmax2 <= 10 eps, reconstruct and the mirror loop from the tail
//     with the Gmax values from before;
//   - rho and obj (:309-327) in position order.
struct Solver {
  // the problem: set by the caller, with t, y, p, C and the starting alpha
  const double* K;
  size_t n;
  int l;
  double eps;
  int64_t max_iter;
  bool shrinking;
  std::vector<int32_t> t;
  std::vector<signed char> y;
  std::vector<double> p, C, alpha;
  // the solve
  int active;
  int64_t iter = 0;
  std::vector<int32_t> aset;
  std::vector<float> QD, Qi, Qn, Qj;
  std::vector<double> G, Gb;
  std::vector<char> st;
  bool unshrunk = false, stopped = false, pending = false;
  // results
  int32_t status = SK_SVM_CONVERGED, n_free = 0, n_bound = 0;
  double rho = 0, obj = 0, r = 0;
  sk_svm_shrink_info info;

  void set_status(int k) { st[k] = alpha[k] >= C[k] ? kUpper : alpha[k] <= 0 ? kLower : kFree; }
  // row i of Q: the int product of the labels times the double, rounded to float
  void row(int i, std::vector<float>& q, int len) const {
    const double* r_ = K + (size_t)t[i] * n;
    const int yi = y[i];
    for (int k = 0; k < len; ++k) q[k] = (float)(yi * y[k] * r_[t[k]]);
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
    std::swap(p[a], p[b]);
    std::swap(C[a], C[b]);
  }

  // The working pair over the active positions; false: optimal.  Leaves row i
  // in Qi.  Solver keeps one maximum of -y G over I_up; Solver_NU one per
  // label (c = 1: y = -1) with that maximiser's row (Qi, Qn), the candidates
  // for j are measured against their own label's, and i is the maximiser of
  // j's label.  With no j, i = -1: the reference reads y[-1] there.
  template <bool NU>
  bool pair(int& i, int& j) {
    double gmax[2] = {-kInf, -kInf}, gmax2[2] = {-kInf, -kInf}, od_min = kInf;
    // jmin and not j in the loop: stores through the reference cost 3 to 9 % of a solve (measured)
    int imax[2] = {-1, -1}, jmin = -1;
    // i: the last maximiser of -y G over I_up
    for (int k = 0; k < active; ++k) {
      const int c = NU && y[k] < 0;
      if (y[k] > 0) {
        if (st[k] != kUpper && -G[k] >= gmax[c]) gmax[c] = -G[k], imax[c] = k;
      } else {
        if (st[k] != kLower && G[k] >= gmax[c]) gmax[c] = G[k], imax[c] = k;
      }
    }
    if (imax[0] >= 0) row(imax[0], Qi, active);
    if (NU && imax[1] >= 0) row(imax[1], Qn, active);
    // j: the last minimiser of the objective's decrease over I_low
    for (int k = 0; k < active; ++k) {
      const int c = NU && y[k] < 0;
      const float* Q = c ? Qn.data() : Qi.data();
      double gd;
      float qf;
      if (y[k] > 0) {
        if (st[k] == kLower) continue;
        gd = gmax[c] + G[k];
        if (G[k] >= gmax2[c]) gmax2[c] = G[k];
        if (!(gd > 0)) continue;  // gd > 0 implies imax[c] >= 0
        qf = Q[imax[c]] + QD[k] - 2 * y[imax[c]] * Q[k];  // float arithmetic
      } else {
        if (st[k] == kUpper) continue;
        gd = gmax[c] - G[k];
        if (-G[k] >= gmax2[c]) gmax2[c] = -G[k];
        if (!(gd > 0)) continue;
        qf = Q[imax[c]] + QD[k] + 2 * y[imax[c]] * Q[k];
      }
      const double qc = qf;
      const double od = qc > 0 ? -(gd * gd) / qc : -(gd * gd) / kTau;
      if (od <= od_min) od_min = od, jmin = k;
    }
    j = jmin;
    if ((NU ? std::max(gmax[0] + gmax2[0], gmax[1] + gmax2[1]) : gmax[0] + gmax2[0]) < eps) return false;
    const int c = NU && j >= 0 && y[j] < 0;
    i = j < 0 ? -1 : imax[c];
    if (c) std::swap(Qi, Qn);
    return true;
  }

  // pair() with the iteration cap and the counters: once max_iter updates
  // have run and a further pair was found (or none can be), this and every
  // later selection report optimal, so the loop below reconstructs the
  // gradient, restores the active set and ends
  template <bool NU>
  bool select(int& i, int& j) {
    if (stopped) return false;
    const bool after_reconstruction = pending;
    pending = false;
    if (!pair<NU>(i, j)) {
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
    for (int k = active; k < l; ++k) G[k] = Gb[k] + p[k];
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

  // k entered or left its upper bound: G_bar -+ C_k Q_k over all l positions
  void update_bar(int k, std::vector<float>& Q, bool was_upper) {
    if (was_upper == (st[k] == kUpper)) return;
    row(k, Q, l);
    const double c = C[k];
    if (was_upper)
      for (int m = 0; m < l; ++m) Gb[m] -= c * Q[m];
    else
      for (int m = 0; m < l; ++m) Gb[m] += c * Q[m];
  }

  // rho: the mean of y G over the free variables, else the bounds' midpoint;
  // Solver_NU: of G per label, rho and r from the two.  Then obj.
  template <bool NU>
  void finish() {
    double ub[2] = {kInf, kInf}, lb[2] = {-kInf, -kInf}, sum[2] = {0, 0};
    int nf[2] = {0, 0};
    for (int k = 0; k < l; ++k) {
      const int c = NU && y[k] < 0;
      const double v = NU ? G[k] : y[k] * G[k];
      if (st[k] == kUpper) ++n_bound;
      if (st[k] == kFree)
        ++nf[c], sum[c] += v;
      else if ((st[k] == kUpper) == (NU || y[k] > 0))
        lb[c] = std::max(lb[c], v);
      else
        ub[c] = std::min(ub[c], v);
    }
    const double r1 = nf[0] > 0 ? sum[0] / nf[0] : (ub[0] + lb[0]) / 2;
    if (NU) {
      const double r2 = nf[1] > 0 ? sum[1] / nf[1] : (ub[1] + lb[1]) / 2;
      r = (r1 + r2) / 2;
      rho = (r1 - r2) / 2;
    } else {
      rho = r1;
    }
    n_free = nf[0] + nf[1];
    double v = 0;
    for (int k = 0; k < l; ++k) v += alpha[k] * (G[k] + p[k]);
    obj = v / 2;
  }

  template <bool NU>
  void solve() {
    active = l;
    info = sk_svm_shrink_info{0, 0, l, 0, 0, 0, 0};
    aset.resize(l), QD.resize(l), Qi.resize(l), Qn.resize(l), Qj.resize(l), st.resize(l);
    G = p;
    Gb.assign(l, 0.0);
    for (int k = 0; k < l; ++k) {
      aset[k] = k;
      QD[k] = (float)K[(size_t)t[k] * n + t[k]];
      set_status(k);
    }
    for (int i = 0; i < l; ++i)
      if (st[i] != kLower) {
        row(i, Qi, l);
        const double a = alpha[i], c = C[i];
        for (int k = 0; k < l; ++k) G[k] += a * Qi[k];
        if (shrinking && st[i] == kUpper)
          for (int k = 0; k < l; ++k) Gb[k] += c * Qi[k];
      }

    const int period = std::min(l, 1000);
    int counter = period + 1;
    for (;;) {
      if (shrinking && --counter == 0) {
        counter = period;
        shrink();
      }
      int i, j;
      if (!select<NU>(i, j)) {
        // with the active set whole, reconstruct and a second selection change nothing
        if (active == l) break;
        reconstruct();
        active = l;
        if (!select<NU>(i, j)) break;
        counter = 1;  // shrink at the next iteration
      }
      ++iter;
      row(j, Qj, active);  // row i is in Qi since the selection
      const double ai0 = alpha[i], aj0 = alpha[j];
      update_pair(y[i] != y[j], Qi[i], Qj[j], Qi[j], G[i], G[j], C[i], C[j], alpha[i], alpha[j]);
      const double dai = alpha[i] - ai0, daj = alpha[j] - aj0;
      for (int k = 0; k < active; ++k) G[k] += Qi[k] * dai + Qj[k] * daj;
      const bool ui = st[i] == kUpper, uj = st[j] == kUpper;
      set_status(i);
      set_status(j);
      if (shrinking) {
        update_bar(i, Qi, ui);
        update_bar(j, Qj, uj);
      }
    }
    finish<NU>();
  }
};

// sum over coef_a != 0 of coef_a K[s][t_a], minus rho, in training order
void decision_values(const double* K, int32_t n, const int32_t* train, int32_t n_train, const double* coef, double rho,
                     const int32_t* test, int32_t n_test, double* dec) {
  for (int q = 0; q < n_test; ++q) {
    const double* r = K + (size_t)test[q] * (size_t)n;
    double sum = 0.0;
    for (int a = 0; a < n_train; ++a)
      if (coef[a] != 0.0) sum += coef[a] * r[train[a]];
    dec[q] = sum - rho;
  }
}

// One job: what svm_train_one leaves (svm.cpp:245-300).  out takes the
// coefficients of the decision function in training order, or for
// sk_svm_train_batch (as_alpha) the alphas themselves.
void solve_job(const double* K, int32_t n, const double* targets, const sk::SvmJob& J, bool shrinking, bool as_alpha,
               double* out, double* dec, sk_svm_task_solution& S, sk_svm_shrink_info& info) {
  Solver s;
  s.K = K, s.n = (size_t)n, s.eps = J.eps, s.max_iter = J.max_iter, s.shrinking = shrinking;
  std::vector<int32_t> ty;
  double Cp = 0, Cn = 0;
  const int L = s.l = sk::svm_task_positions(targets, J, ty, s.p, s.alpha, &Cp, &Cn);
  s.t.resize(L), s.y.resize(L), s.C.resize(L);
  for (int k = 0; k < L; ++k) {
    s.t[k] = ty[k] >> 1;
    s.y[k] = (ty[k] & 1) ? +1 : -1;
    s.C[k] = s.y[k] > 0 ? Cp : Cn;
  }
  if (sk::svm_type_is_nu(J.svm_type)) s.solve<true>();
  else s.solve<false>();
  S = sk_svm_task_solution{s.rho, s.obj, s.iter, s.status, s.n_free, s.n_bound, s.r};
  info = s.info;

  const int l = J.n_train;
  std::vector<double> a(L);  // the alphas back at the positions they started at
  for (int k = 0; k < L; ++k) a[s.aset[k]] = s.alpha[k];
  auto y0 = [&](int k) { return (ty[k] & 1) ? +1 : -1; };
  if (J.svm_type == SK_SVM_C_SVC) {
    for (int k = 0; k < l; ++k) out[k] = a[k] * y0(k);
  } else if (J.svm_type == SK_SVM_NU_SVC) {
    const double r = s.r;
    for (int k = 0; k < l; ++k) out[k] = a[k] * (y0(k) / r);
    S.rho /= r;
    S.obj /= (r * r);
  } else if (J.svm_type == SK_SVM_ONE_CLASS) {
    for (int k = 0; k < l; ++k) out[k] = a[k];
  } else {
    for (int k = 0; k < l; ++k) out[k] = a[k] - a[k + l];
  }
  decision_values(K, n, J.train, l, out, S.rho, J.test, J.n_test, dec);
  if (as_alpha) std::copy(a.begin(), a.begin() + l, out);
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

// The host path of both calls: the checks, the outputs' offsets, one job per
// pool slot.  keep(p, S, info) stores job p's records in the caller's arrays.
template <class Keep>
int run_jobs(const sk::SvmCall& call, const double* gram, int32_t n, const double* targets,
             const std::vector<sk::SvmJob>& jobs, int32_t n_jobs, int32_t n_threads, bool shrinking, double* out,
             double* dec_out, const void* solutions, Keep keep) {
  std::string err;
  int64_t st = 0, ss = 0;
  const int rc = sk::svm_check_jobs(call, gram, n, targets, jobs, n_jobs, out, dec_out, solutions, false, &st, &ss, err);
  if (rc) return rc;
  if (n_threads < 0) return SK_ERR_INVALID;
  std::vector<int64_t> aoff(n_jobs + 1, 0), doff(n_jobs + 1, 0);
  for (int p = 0; p < n_jobs; ++p) {
    if (shrinking && jobs[p].svm_type != SK_SVM_C_SVC) return SK_ERR_UNSUPPORTED;  // do_shrinking of Solver only
    aoff[p + 1] = aoff[p] + jobs[p].n_train;
    doff[p + 1] = doff[p] + jobs[p].n_test;
  }
  return run_pool(n_jobs, n_threads, [&](int p) {
    sk_svm_task_solution S;
    sk_svm_shrink_info info;
    solve_job(gram, n, targets, jobs[p], shrinking, !call.typed, out + aoff[p], dec_out ? dec_out + doff[p] : nullptr,
              S, info);
    keep(p, S, info);
  });
}

}  // namespace

namespace sk {

int svm_task_positions(const double* targets, const SvmJob& J, std::vector<int32_t>& ty, std::vector<double>& p,
                       std::vector<double>& alpha0, double* Cp, double* Cn) {
  const int l = J.n_train;
  const size_t at = ty.size();
  const bool svr = svm_type_is_svr(J.svm_type);
  const int L = svr ? 2 * l : l;
  ty.resize(at + L), p.resize(at + L), alpha0.resize(at + L);
  int32_t* y_ = ty.data() + at;
  double* p_ = p.data() + at;
  double* a_ = alpha0.data() + at;
  *Cp = *Cn = svr ? J.Cp : 1.0;
  if (J.svm_type == SK_SVM_C_SVC) {
    for (int k = 0; k < l; ++k) {
      a_[k] = 0;
      p_[k] = -1;
      y_[k] = (J.train[k] << 1) | (targets[J.train[k]] > 0 ? 1 : 0);
    }
    *Cp = J.Cp, *Cn = J.Cn;
  } else if (J.svm_type == SK_SVM_NU_SVC) {
    const double nu = J.nu;
    double sum_pos = nu * l / 2, sum_neg = nu * l / 2;
    for (int k = 0; k < l; ++k) {
      const bool pos = targets[J.train[k]] > 0;
      double& sum = pos ? sum_pos : sum_neg;
      a_[k] = std::min(1.0, sum);
      sum -= a_[k];
      p_[k] = 0;
      y_[k] = (J.train[k] << 1) | (pos ? 1 : 0);
    }
  } else if (J.svm_type == SK_SVM_ONE_CLASS) {
    const int m = (int)(J.nu * l);  // alphas at the upper bound
    for (int k = 0; k < l; ++k) {
      a_[k] = k < m ? 1 : 0;
      p_[k] = 0;
      y_[k] = (J.train[k] << 1) | 1;
    }
    if (m < l) a_[m] = J.nu * l - m;
  } else if (J.svm_type == SK_SVM_EPSILON_SVR) {
    for (int k = 0; k < l; ++k) {
      const double v = targets[J.train[k]];
      a_[k] = a_[k + l] = 0;
      p_[k] = J.p - v;
      p_[k + l] = J.p + v;
      y_[k] = (J.train[k] << 1) | 1;
      y_[k + l] = J.train[k] << 1;
    }
  } else {  // SK_SVM_NU_SVR
    const double C = J.Cp;
    double sum = C * J.nu * l / 2;
    for (int k = 0; k < l; ++k) {
      const double v = targets[J.train[k]];
      a_[k] = a_[k + l] = std::min(sum, C);
      sum -= a_[k];
      p_[k] = -v;
      p_[k + l] = v;
      y_[k] = (J.train[k] << 1) | 1;
      y_[k + l] = J.train[k] << 1;
    }
  }
  return L;
}

// sk_svm_train_batch tests C before max_iter, sk_svm_solve_batch after it,
// and each call words its over-long list in its own way; all else is shared.
int svm_check_jobs(const SvmCall& call, const double* gram, int32_t n, const double* targets,
                   const std::vector<SvmJob>& jobs, int32_t n_jobs, const double* out, const double* dec_out,
                   const void* solutions, bool on_gpu, int64_t* sum_train, int64_t* sum_test, std::string& err) {
  const std::string who = std::string(call.name) + ": ";
  auto bad = [&](int p, const char* what) {
    err = who + call.noun + " " + std::to_string(p) + ": " + what;
    return (int)SK_ERR_INVALID;
  };
  if (!gram || (!call.typed && !targets) || n < 1 || n_jobs < 0 || jobs.size() != (size_t)n_jobs || !out ||
      (n_jobs && !solutions)) {
    err = who + "null or empty argument";
    return SK_ERR_INVALID;
  }
  int64_t st = 0, ss = 0;
  for (int p = 0; p < n_jobs; ++p) {
    const SvmJob& J = jobs[p];
    const int ty = J.svm_type;
    const bool bad_C = (ty == SK_SVM_C_SVC || svm_type_is_svr(ty)) && (!(J.Cp > 0) || !(J.Cn > 0));
    if (ty < SK_SVM_C_SVC || ty > SK_SVM_NU_SVR) return bad(p, "unknown svm type");
    if (ty != SK_SVM_ONE_CLASS && !targets) return bad(p, "targets is null");
    if (J.n_train < 2 || !J.train) return bad(p, "n_train < 2");
    if (J.n_test < 0 || (J.n_test && !J.test)) return bad(p, "test list");
    if (!(J.eps > 0)) return bad(p, "eps <= 0");
    if (!call.typed && bad_C) return bad(p, "C <= 0");
    if (J.max_iter < 1) return bad(p, "max_iter < 1");
    if (bad_C) return bad(p, "C <= 0");
    if ((ty == SK_SVM_NU_SVC || ty == SK_SVM_ONE_CLASS || ty == SK_SVM_NU_SVR) && !(J.nu > 0 && J.nu <= 1))
      return bad(p, "nu <= 0 or nu > 1");
    if (ty == SK_SVM_EPSILON_SVR && !(J.p >= 0)) return bad(p, "p < 0");
    int64_t np = 0, nn = 0;
    for (int k = 0; k < J.n_train; ++k) {
      const int32_t t = J.train[k];
      if (t < 0 || t >= n) return bad(p, "training index outside [0, n)");
      if (svm_type_is_svr(ty)) {
        if (!std::isfinite(targets[t])) return bad(p, "a target that is not finite");
      } else if (ty != SK_SVM_ONE_CLASS) {
        ++(targets[t] > 0 ? np : nn);
      }
    }
    for (int k = 0; k < J.n_test; ++k)
      if (J.test[k] < 0 || J.test[k] >= n) return bad(p, "test index outside [0, n)");
    if (ty == SK_SVM_C_SVC || ty == SK_SVM_NU_SVC) {
      if (!np || !nn) return bad(p, "training list with one class only");
      if (ty == SK_SVM_NU_SVC && J.nu * (double)(np + nn) / 2 > (double)std::min(np, nn))
        return bad(p, "specified nu is infeasible");
    }
    st += J.n_train;
    ss += J.n_test;
  }
  if (ss && !dec_out) {
    err = who + "dec_out is null";
    return SK_ERR_INVALID;
  }
  if (on_gpu)
    for (int p = 0; p < n_jobs; ++p) {
      const int max_train = svm_type_max_train(jobs[p].svm_type);
      if (jobs[p].n_train > max_train) {
        err = who + call.noun + " " + std::to_string(p) + ": n_train " + std::to_string(jobs[p].n_train) +
              " over the GPU solver's " + std::to_string(max_train) + (call.typed ? " for its type" : "");
        return SK_ERR_UNSUPPORTED;
      }
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
    return run_jobs(sk::kSvmTrainBatch, gram, n, labels, sk::svm_jobs(problems, n_problems), n_problems, n_threads,
                    shrinking != 0, alpha_out, dec_out, solutions,
                    [&](int p, const sk_svm_task_solution& S, const sk_svm_shrink_info& si) {
                      solutions[p] = sk_svm_solution{S.rho, S.obj, S.iterations, S.status, S.n_free, S.n_bound};
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
    return run_jobs(sk::kSvmSolveBatch, gram, n, targets, sk::svm_jobs(tasks, n_tasks), n_tasks, n_threads, false,
                    coef_out, dec_out, solutions,
                    [&](int p, const sk_svm_task_solution& S, const sk_svm_shrink_info&) { solutions[p] = S; });
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
