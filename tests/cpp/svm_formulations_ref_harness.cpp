// Reference harness for tests/golden/svm_formulations.json: runs the
// reference's own solve_nu_svc, solve_one_class, solve_epsilon_svr and
// solve_nu_svr (libsvm/svm.cpp, with libsvm/solver.cpp and libsvm/qmatrix.cpp,
// all three included in place) with shrinking = 0 on the tasks
// tools/make_golden_svm_formulations.py describes, and prints what
// svm_train_one would keep: the coefficients, rho, obj and r as C99 hex
// floats, the iteration count and the solver's counts of positions at the
// upper bound and strictly inside.  Built into a temporary directory by that
// tool with
//   g++ -O2 -ffp-contract=off -I<reference> -I<reference>/libsvm
// and never kept.
//
// The three files define the same static helpers (clone, info, info_flush),
// renamed by macro below.  svm.cpp also defines global min, max and swap
// templates, which would be ambiguous next to the other two files'
// using-declarations of std's: its swap is renamed, and its min and max, which
// it guards with #ifndef so that a macro can stand in for them, are macros
// for the standard library's (what solver.cpp and qmatrix.cpp use).
//
// Solver and Solver_NU are replaced by macro, inside svm.cpp only, with
// subclasses that only watch: select_working_set counts the selections that
// found a pair (the iterations) and, once `cap` of them have run and a
// further pair was found, reports optimal from then on, so a capped record is
// the reference's own state after exactly that many updates; calculate_rho
// counts the positions by alpha_status before it hands on.
//
// Input (text): n_grams, then per Gram "n", n class labels, n targets and n*n
// entries (hex floats); n_tasks, then per task
//   gram svm_type l C nu p eps cap, l training indices
// Output per task: "P iters capped n_bound n_free", l coefficients, "rho obj r".
#include <ctype.h>
#include <float.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

// Solver_NU keeps its two hooks private; the watching subclass has to call them
#define private protected
#include "libsvm/solver.h"
#undef private

#define clone clone_q
#include "libsvm/qmatrix.cpp"
#undef clone
#define info info_solver
#define info_flush info_flush_solver
#include "libsvm/solver.cpp"
#undef info
#undef info_flush

namespace {

struct Watch {
  long cap = 0, iters = 0;
  bool capped = false;
  int n_bound = 0, n_free = 0;
} g_watch;

template <class Base>
class Watching : public Base {
 protected:
  int select_working_set(int& i, int& j) {
    if (g_watch.capped) return 1;
    if (Base::select_working_set(i, j)) return 1;
    if (g_watch.iters == g_watch.cap) {
      g_watch.capped = true;
      return 1;
    }
    ++g_watch.iters;
    return 0;
  }
  double calculate_rho() {
    g_watch.n_bound = g_watch.n_free = 0;
    for (int k = 0; k < this->l; ++k) {
      if (this->is_upper_bound(k)) ++g_watch.n_bound;
      else if (!this->is_lower_bound(k)) ++g_watch.n_free;
    }
    return Base::calculate_rho();
  }
};
typedef Watching<Solver> WatchingSolver;
typedef Watching<Solver_NU> WatchingSolverNU;

}  // namespace

#define min std::min
#define max std::max
#define swap swap_svm
#define Solver_NU WatchingSolverNU
#define Solver WatchingSolver
#include "libsvm/svm.cpp"
#undef Solver
#undef Solver_NU
#undef swap
#undef max
#undef min

namespace {

struct Gram {
  int n = 0;
  std::vector<double> K, y, target;
  std::vector<svm_node> nodes;  // per example: {0, serial}, {c + 1, K[r][c]}..., {-1, 0}
  svm_node* row(int r) { return nodes.data() + (size_t)r * (n + 2); }
  void index() {
    nodes.resize((size_t)n * (n + 2));
    for (int r = 0; r < n; ++r) {
      svm_node* x = row(r);
      x[0].index = 0, x[0].value = r + 1;
      for (int c = 0; c < n; ++c) x[c + 1].index = c + 1, x[c + 1].value = K[(size_t)r * n + c];
      x[n + 1].index = -1, x[n + 1].value = 0;
    }
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int n_grams = 0;
  if (fscanf(f, "%d", &n_grams) != 1) return 2;
  std::vector<Gram> grams(n_grams);
  for (Gram& g : grams) {
    if (fscanf(f, "%d", &g.n) != 1) return 2;
    g.y.resize(g.n), g.target.resize(g.n), g.K.resize((size_t)g.n * g.n);
    for (double& v : g.y)
      if (fscanf(f, "%lf", &v) != 1) return 2;
    for (double& v : g.target)
      if (fscanf(f, "%la", &v) != 1) return 2;
    for (double& v : g.K)
      if (fscanf(f, "%la", &v) != 1) return 2;
    g.index();
  }
  int n_tasks = 0;
  if (fscanf(f, "%d", &n_tasks) != 1) return 2;
  for (int p = 0; p < n_tasks; ++p) {
    int gi, type, l;
    double C, nu, eps_tube, eps;
    long cap;
    if (fscanf(f, "%d %d %d %la %la %la %la %ld", &gi, &type, &l, &C, &nu, &eps_tube, &eps, &cap) != 8) return 2;
    Gram& g = grams[gi];
    std::vector<svm_node*> x(l);
    std::vector<double> yv(l), coef(l, 0.0);
    for (int k = 0; k < l; ++k) {
      int t;
      if (fscanf(f, "%d", &t) != 1 || t < 0 || t >= g.n) return 2;
      x[k] = g.row(t);
      yv[k] = (type == EPSILON_SVR || type == NU_SVR) ? g.target[t] : g.y[t];
    }
    svm_problem prob;
    prob.l = l, prob.y = yv.data(), prob.x = x.data();
    svm_parameter param;
    memset(&param, 0, sizeof(param));
    param.svm_type = type, param.kernel_type = PRECOMPUTED, param.cache_size = 40, param.eps = eps;
    param.C = C, param.nu = nu, param.p = eps_tube, param.shrinking = 0;
    g_watch = Watch();
    g_watch.cap = cap;
    Solver::SolutionInfo si;
    si.r = 0;  // the plain solver leaves it unset
    switch (type) {
      case NU_SVC: solve_nu_svc(&prob, &param, coef.data(), &si); break;
      case ONE_CLASS: solve_one_class(&prob, &param, coef.data(), &si); break;
      case EPSILON_SVR: solve_epsilon_svr(&prob, &param, coef.data(), &si); break;
      case NU_SVR: solve_nu_svr(&prob, &param, coef.data(), &si); break;
      default: return 2;
    }
    printf("P %ld %d %d %d\n", g_watch.iters, g_watch.capped ? 1 : 0, g_watch.n_bound, g_watch.n_free);
    for (int k = 0; k < l; ++k) printf("%a%c", coef[k], k + 1 < l ? ' ' : '\n');
    printf("%a %a %a\n", si.rho, si.obj, si.r);
  }
  return 0;
}
