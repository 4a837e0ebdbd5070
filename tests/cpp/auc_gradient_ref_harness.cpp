// Reference harness for tests/golden/auc_gradient.json: includes the
// reference's optimizer/gradient.cpp, libsvm/solver.cpp and libsvm/qmatrix.cpp
// in place and calls gradient.cpp's own stage functions -- compute_delta
// (through a subclass: it is protected), find_support_vectors, solve_d,
// calculate_gradient_c, calculate_gradient_p -- on the problems
// tools/make_golden_auc_gradient.py describes, printing C99 hex floats.
// Built into a temporary directory by that tool with
//   g++ -O2 -ffp-contract=off -I tests/cpp/ublas_standin
//       -I oracle/ref_shim/standin -I<reference> -I<reference>/libsvm
// and never kept.  Boost is replaced by the stand-ins under those two
// directories, so what is pinned is the reference's code over the stand-ins'
// accumulation order (ascending index from zero), not over Boost itself.
//
// A "natural" problem first runs the reference's Solver::Solve with
// shrinking 0 (as tests/cpp/svm_train_ref_harness.cpp does) and the
// reference's svm_predict for the decision values; a crafted one reads
// alpha, b and the decision values.  The products the conjugate gradient
// forms are counted by the stand-in's prod: calls inside solve_d minus the
// first one (A x).  For natural problems the whole compute() (which
// hardcodes shrinking = 1) is also run; its values are recorded, not pinned.
//
// Input (text): n_matrices, then per matrix "n" and n*n hex floats;
//   n_problems, then per problem
//     k_matrix n_params [g_matrix ...] l m C natural eps
//     n labels; l training indices; m test indices;
//     crafted only: l alphas, b, m decision values
// Output per problem:
//   "A" l alphas, b, m decision values
//   "F" f, m deltas
//   "S" n_free n_bound products
//   "D" the n_free + 1 entries of d_u (none when n_free = 0)
//   "G" cg, fg[0..n_params)
//   "X" f cg fg... of compute()   (natural only)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// both libsvm files define the same clone() template
#define clone clone_q
#include "libsvm/qmatrix.cpp"
#undef clone
#include "libsvm/solver.cpp"
#include "optimizer/gradient.cpp"

namespace {

struct DeltaAccess : public GradientComputationAUC {
  DeltaAccess(const std::vector<int>& y, const std::vector<uint>& tr, const std::vector<uint>& ts)
      : GradientComputationAUC(y, tr, ts) {}
  double delta(const std::vector<double>& dec, std::vector<double>& out) const { return compute_delta(dec, out); }
};

bool read_doubles(FILE* f, std::vector<double>& v) {
  for (double& x : v)
    if (std::fscanf(f, "%la", &x) != 1) return false;
  return true;
}

void print_doubles(const char* tag, const std::vector<double>& v) {
  std::printf("%s", tag);
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_mats = 0;
  if (std::fscanf(f, "%d", &n_mats) != 1) return 2;
  std::vector<std::vector<double> > mats(n_mats);
  std::vector<int> dims(n_mats);
  for (int k = 0; k < n_mats; ++k) {
    if (std::fscanf(f, "%d", &dims[k]) != 1) return 2;
    mats[k].resize((size_t)dims[k] * dims[k]);
    if (!read_doubles(f, mats[k])) return 2;
  }
  int n_prob = 0;
  if (std::fscanf(f, "%d", &n_prob) != 1) return 2;
  for (int p = 0; p < n_prob; ++p) {
    int ki, n_params;
    if (std::fscanf(f, "%d %d", &ki, &n_params) != 2 || ki < 0 || ki >= n_mats) return 2;
    const int n = dims[ki];
    std::vector<int> gi(n_params);
    for (int& g : gi)
      if (std::fscanf(f, "%d", &g) != 1 || g < 0 || g >= n_mats || dims[g] != n) return 2;
    int l, m, natural;
    double C, eps;
    if (std::fscanf(f, "%d %d %la %d %la", &l, &m, &C, &natural, &eps) != 5) return 2;
    std::vector<int> y(n);
    for (int& v : y)
      if (std::fscanf(f, "%d", &v) != 1) return 2;
    std::vector<uint> tr(l), ts(m);
    for (uint& v : tr)
      if (std::fscanf(f, "%u", &v) != 1 || v >= (uint)n) return 2;
    for (uint& v : ts)
      if (std::fscanf(f, "%u", &v) != 1 || v >= (uint)n) return 2;

    Kmat kmat(boost::extents[n][n]);
    // compute() asserts on g[0], so the array never has fewer than one matrix
    Gmat gmat(boost::extents[n_params ? n_params : 1][n][n]);
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c) {
        kmat[r][c] = mats[ki][(size_t)r * n + c];
        for (int q = 0; q < n_params; ++q) gmat[q][r][c] = mats[gi[q]][(size_t)r * n + c];
      }

    std::vector<double> alpha(l), dec(m);
    double b = 0.0;
    if (natural) {
      // the reference's svm_train (gradient.cpp) with shrinking 0 in place of its hardcoded 1
      svm_problem* prob = make_problem(tr, y, kmat);
      svm_parameter param;
      std::memset(&param, 0, sizeof(param));
      param.svm_type = C_SVC, param.kernel_type = PRECOMPUTED, param.cache_size = 40, param.eps = eps;
      param.C = C;
      std::vector<double> minus_ones(l, -1.0);
      std::vector<schar> ys(l);
      for (int k = 0; k < l; ++k) alpha[k] = 0, ys[k] = prob->y[k] > 0.0 ? +1 : -1;
      Solver s;
      Solver::SolutionInfo si;
      s.Solve(l, SVC_Q(*prob, param, ys.data()), minus_ones.data(), ys.data(), alpha.data(), C, C, eps, &si, 0);
      b = si.rho;
      for (int k = 0; k < m; ++k) {
        svm_node* x = make_node(kmat, ts[k]);
        dec[k] = svm_predict(prob, x, alpha.data(), b);
        destroy_node(x);
      }
      destroy_problem(prob);
    } else {
      double bb;
      if (!read_doubles(f, alpha) || std::fscanf(f, "%la", &bb) != 1 || !read_doubles(f, dec)) return 2;
      b = bb;
    }
    std::printf("A");
    for (double v : alpha) std::printf(" %a", v);
    std::printf(" %a", b);
    for (double v : dec) std::printf(" %a", v);
    std::printf("\n");

    DeltaAccess gc(y, tr, ts);
    std::vector<double> delta(m);
    const double fv = gc.delta(dec, delta);
    std::printf("F %a", fv);
    for (double v : delta) std::printf(" %a", v);
    std::printf("\n");

    std::vector<uint> u_idx, c_idx, z_idx;
    bnu::vector<double> alpha_u, d_u;
    find_support_vectors(tr, C, alpha, alpha_u, u_idx, c_idx, z_idx);
    const long before = bnu::standin_prod_calls();
    solve_d(kmat, y, ts, u_idx, delta, d_u);
    const long calls = bnu::standin_prod_calls() - before;
    std::printf("S %d %d %ld\n", (int)u_idx.size(), (int)c_idx.size(), calls > 0 ? calls - 1 : 0L);
    std::printf("D");
    for (size_t k = 0; k != d_u.size(); ++k) std::printf(" %a", d_u(k));
    std::printf("\n");
    const double cg = calculate_gradient_c(kmat, y, u_idx, c_idx, ts, d_u, delta);
    std::printf("G %a", cg);
    for (int q = 0; q < n_params; ++q)
      std::printf(" %a", calculate_gradient_p(kmat, gmat, y, (uint)q, C, u_idx, c_idx, tr, ts, d_u, delta, alpha,
                                               alpha_u, b));
    std::printf("\n");

    if (natural) {
      std::vector<double> fg(n_params);
      double cgx = 0.0;
      const double fx = gc.compute(kmat, gmat, C, fg, cgx, eps);
      std::printf("X %a %a", fx, cgx);
      for (double v : fg) std::printf(" %a", v);
      std::printf("\n");
    }
  }
  return 0;
}
