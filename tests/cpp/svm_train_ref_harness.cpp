// Reference harness for tests/golden/svm_train.json: runs the reference's own
// SMO solver (libsvm/solver.cpp, libsvm/qmatrix.cpp, included in place) on the
// problems tools/make_golden_svm_train.py describes and prints alphas, rho and
// obj as C99 hex floats.  Built into a temporary directory by that tool with
//   g++ -O2 -ffp-contract=off -I<reference> -I<reference>/libsvm
// and never kept.
//
// The iteration cap and the iteration count come from a subclass that
// overrides the virtual select_working_set: it counts the selections that
// found a pair and reports "optimal" once `cap` iterations have run, so the
// capped record is the reference's own state after exactly that many updates.
//
// Input (text):
//   n_grams, then per Gram either
//     I seed n d shift indef dup     integer Gram, generated here (int_gram)
//     S n, n labels, n*n hex floats  stored Gram
//   n_problems, then per problem
//     gram l Cp Cn eps cap, l training indices
// Output: per integer Gram "G <sum of entries> <labels>"; per problem
//   "P iters capped seconds", l alphas, "rho obj" (shrinking 0), then
//   "rho obj seconds" with shrinking 1 (no cap).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// both files define the same clone() template
#define clone clone_q
#include "libsvm/qmatrix.cpp"
#undef clone
#include "libsvm/solver.cpp"

namespace {

struct Gram {
  int n = 0;
  std::vector<double> K, y;
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

uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// K = A S A^T / 2^shift: A n x d of integers in [-3, 3] drawn row by row, S
// the identity or (indef) the alternating signs +1, -1, ...; then the labels,
// +1 / -1 by one draw each, the first two forced to +1, -1.  dup: example 1
// is example 0 again (with the opposite label).
void int_gram(Gram& g, uint64_t seed, int n, int d, int shift, int indef, int dup) {
  std::vector<int> A((size_t)n * d);
  uint64_t s = seed;
  for (auto& a : A) a = (int)(splitmix64(s) % 7) - 3;
  if (dup)
    for (int c = 0; c < d; ++c) A[d + c] = A[c];
  g.n = n;
  g.K.resize((size_t)n * n);
  g.y.resize(n);
  for (int r = 0; r < n; ++r) g.y[r] = (splitmix64(s) & 1) ? 1.0 : -1.0;
  g.y[0] = 1.0, g.y[1] = -1.0;
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) {
      long v = 0;
      for (int k = 0; k < d; ++k) v += (long)((indef && (k & 1)) ? -1 : 1) * A[r * d + k] * A[c * d + k];
      g.K[(size_t)r * n + c] = std::ldexp((double)v, -shift);
    }
}

class CountingSolver : public Solver {
 public:
  long cap = 0, iters = 0;
  bool capped = false;

 protected:
  int select_working_set(int& i, int& j) {
    if (capped) return 1;
    if (Solver::select_working_set(i, j)) return 1;
    if (iters == cap) {
      capped = true;
      return 1;
    }
    ++iters;
    return 0;
  }
};

double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_grams = 0;
  if (std::fscanf(f, "%d", &n_grams) != 1) return 2;
  std::vector<Gram> grams(n_grams);
  for (Gram& g : grams) {
    char kind[4];
    if (std::fscanf(f, "%3s", kind) != 1) return 2;
    if (kind[0] == 'I') {
      unsigned long long seed;
      int n, d, shift, indef, dup;
      if (std::fscanf(f, "%llu %d %d %d %d %d", &seed, &n, &d, &shift, &indef, &dup) != 6) return 2;
      int_gram(g, seed, n, d, shift, indef, dup);
      double sum = 0;
      for (double v : g.K) sum += v;
      std::printf("G %a", sum);
      for (double v : g.y) std::printf(" %d", (int)v);
      std::printf("\n");
    } else {
      if (std::fscanf(f, "%d", &g.n) != 1) return 2;
      g.y.resize(g.n);
      g.K.resize((size_t)g.n * g.n);
      for (double& v : g.y)
        if (std::fscanf(f, "%lf", &v) != 1) return 2;
      for (double& v : g.K)
        if (std::fscanf(f, "%la", &v) != 1) return 2;
    }
    g.index();
  }
  int n_prob = 0;
  if (std::fscanf(f, "%d", &n_prob) != 1) return 2;
  for (int p = 0; p < n_prob; ++p) {
    int gi, l;
    double Cp, Cn, eps;
    long cap;
    if (std::fscanf(f, "%d %d %la %la %la %ld", &gi, &l, &Cp, &Cn, &eps, &cap) != 6) return 2;
    Gram& g = grams[gi];
    std::vector<svm_node*> x(l);
    std::vector<double> yv(l), alpha(l), minus_ones(l, -1.0);
    std::vector<schar> y(l);
    for (int k = 0; k < l; ++k) {
      int t;
      if (std::fscanf(f, "%d", &t) != 1 || t < 0 || t >= g.n) return 2;
      x[k] = g.row(t);
      yv[k] = g.y[t];
      y[k] = yv[k] > 0 ? +1 : -1;
    }
    svm_problem prob;
    prob.l = l, prob.y = yv.data(), prob.x = x.data();
    svm_parameter param;
    std::memset(&param, 0, sizeof(param));
    param.svm_type = C_SVC, param.kernel_type = PRECOMPUTED, param.cache_size = 40, param.eps = eps;
    for (int shrinking = 0; shrinking < 2; ++shrinking) {
      std::fill(alpha.begin(), alpha.end(), 0.0);
      CountingSolver s;
      s.cap = shrinking ? 2000000000L : cap;
      Solver::SolutionInfo si;
      const double t0 = now();
      s.Solve(l, SVC_Q(prob, param, y.data()), minus_ones.data(), y.data(), alpha.data(), Cp, Cn, eps, &si,
              shrinking);
      const double dt = now() - t0;
      if (!shrinking) {
        std::printf("P %ld %d %.6f\n", s.iters, s.capped ? 1 : 0, dt);
        for (int k = 0; k < l; ++k) std::printf("%a%c", alpha[k], k + 1 < l ? ' ' : '\n');
        std::printf("%a %a\n", si.rho, si.obj);
      } else {
        std::printf("%a %a %.6f\n", si.rho, si.obj, dt);
      }
    }
  }
  return 0;
}
