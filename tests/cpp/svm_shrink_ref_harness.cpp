// Reference harness for tests/golden/svm_train_shrink.json: runs the
// reference's own SMO solver (libsvm/solver.cpp, libsvm/qmatrix.cpp, included
// in place) with shrinking = 1 on the problems tools/make_golden_svm_shrink.py
// describes and prints alphas, rho and obj as C99 hex floats, the iteration
// count and the counters of sk_svm_shrink_info.  Built into a temporary
// directory by that tool with
//   g++ -O2 -ffp-contract=off -I<reference> -I<reference>/libsvm
// and never kept.
//
// A subclass overrides the solver's two virtual hooks and only watches:
//   select_working_set  counts the selections that found a pair (the
//     iterations) and the ones that reported optimal while the active set was
//     shrunk (reconstructions; resumed when the selection after the
//     reconstruction found a pair).  The cap: once `cap` iterations have run
//     and a further pair was found, this and every later selection report
//     optimal, so the solver reconstructs the gradient, restores the active
//     set and leaves its loop: the capped record is the reference's own state
//     after exactly that many updates.
//   do_shrinking  counts the calls and compares the active size before and
//     after each: a call shrank when it left fewer active positions than it
//     found; the call in which the `unshrinked` flag turns true ran the
//     unshrink branch, and regrew the set when it left more than it found.
//
// Input (text), as tests/cpp/svm_train_ref_harness.cpp takes it:
//   n_grams, then per Gram either
//     I seed n d shift indef dup     integer Gram, generated here (int_gram)
//     S n, n labels, n*n hex floats  stored Gram
//   n_problems, then per problem
//     gram l Cp Cn eps cap, l training indices
// Output: per integer Gram "G <sum of entries> <labels>"; per problem
//   "P iters capped capped_active shrink_calls shrunk_calls min_active unshrunk regrown
//    reconstructions resumed", l alphas, "rho obj".
#include <algorithm>
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

// the generator of tests/cpp/svm_train_ref_harness.cpp (tests/svm_ref.py: int_gram)
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

class WatchingSolver : public Solver {
 public:
  long cap = 0, iters = 0;
  bool capped = false, pending = false;
  int shrink_calls = 0, shrunk_calls = 0, min_active = -1, unshrunk = 0, regrown = 0, reconstructions = 0,
      resumed = 0, capped_active = 0;

 protected:
  int select_working_set(int& i, int& j) {
    if (capped) return 1;
    const bool after_reconstruction = pending;
    pending = false;
    if (Solver::select_working_set(i, j)) {
      if (active_size < l) ++reconstructions, pending = true;
      return 1;
    }
    if (iters == cap) {
      capped = true;
      capped_active = active_size;
      return 1;
    }
    if (after_reconstruction) ++resumed;
    ++iters;
    return 0;
  }

  void do_shrinking() {
    if (min_active < 0) min_active = l;
    ++shrink_calls;
    const int before = active_size;
    const bool was = unshrinked;
    Solver::do_shrinking();
    if (active_size < before) ++shrunk_calls;
    min_active = std::min(min_active, active_size);
    if (unshrinked && !was) {
      unshrunk = 1;
      if (active_size > before) regrown = 1;
    }
  }
};

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
    std::vector<double> yv(l), alpha(l, 0.0), minus_ones(l, -1.0);
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
    WatchingSolver s;
    s.cap = cap;
    Solver::SolutionInfo si;
    s.Solve(l, SVC_Q(prob, param, y.data()), minus_ones.data(), y.data(), alpha.data(), Cp, Cn, eps, &si, 1);
    std::printf("P %ld %d %d %d %d %d %d %d %d %d\n", s.iters, s.capped ? 1 : 0, s.capped_active, s.shrink_calls, s.shrunk_calls,
                s.min_active < 0 ? l : s.min_active, s.unshrunk, s.regrown, s.reconstructions, s.resumed);
    for (int k = 0; k < l; ++k) std::printf("%a%c", alpha[k], k + 1 < l ? ' ' : '\n');
    std::printf("%a %a\n", si.rho, si.obj);
  }
  return 0;
}
