// Reference harness for tests/golden/feature_gram.json and .npz: includes one of the
// reference's optimizer/rbf_kernel.cpp, poly_kernel.cpp, sigmoid_kernel.cpp in
// place (each defines static dot / kernel, so one binary per kernel:
// -DSK_FEAT_KERNEL=0 RBF, 1 polynomial, 2 sigmoid) and calls its own read_data,
// dot and calculate_matrix on a feature file, printing C99 hex floats.  Built
// into a temporary directory by tools/make_golden_feature_gram.py with
//   g++ -O2 -ffp-contract=off -DSK_FEAT_KERNEL=k -I tests/cpp/feature_standin
//       -I oracle/ref_shim/standin -I<reference> -I<reference>/optimizer
// and never kept.  Boost is replaced by the project's stand-ins (multi_array,
// shared_array), which hold no arithmetic.
//
//   harness feature-file degree p0 [p1]
// Output: "L" the labels; per example "V" index:value ...; "D" the upper
// triangle (i <= j, row by row) of dot(); "K", "G0" and (two parameters) "G1"
// the upper triangles of calculate_matrix's kmat and gmat.  The lower
// triangles are checked to mirror the upper ones.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#if SK_FEAT_KERNEL == 0
#include "optimizer/rbf_kernel.cpp"
typedef RBFKernel CM;
#elif SK_FEAT_KERNEL == 1
#include "optimizer/poly_kernel.cpp"
typedef PolyKernel CM;
#else
#include "optimizer/sigmoid_kernel.cpp"
typedef SigmoidKernel CM;
#endif

namespace {
template <class A>
void upper(const char* tag, const A& m, size_t n) {
  std::printf("%s", tag);
  for (size_t i = 0; i != n; ++i)
    for (size_t j = i; j != n; ++j) {
      if (m[i][j] != m[j][i] && !(m[i][j] != m[i][j])) {
        std::fprintf(stderr, "%s is not symmetric at %zu %zu\n", tag, i, j);
        std::exit(2);
      }
      std::printf(" %a", (double)m[i][j]);
    }
  std::printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) return 1;
  std::ifstream is(argv[1]);
  std::vector<int> labels;
  std::vector<CM::Data> vec;
  CM::read_data(is, labels, vec);
  const size_t n = vec.size();
  std::vector<double> param;
  for (int a = 3; a < argc; ++a) param.push_back(std::strtod(argv[a], 0));
  std::printf("L");
  for (size_t i = 0; i != n; ++i) std::printf(" %d", labels[i]);
  std::printf("\n");
  for (size_t i = 0; i != n; ++i) {
    std::printf("V");
    for (const svm_node* p = &vec[i][0]; p->index != -1; ++p) std::printf(" %d:%a", p->index, p->value);
    std::printf("\n");
  }
  Kmat d(boost::extents[n][n]);
  for (size_t i = 0; i != n; ++i)
    for (size_t j = 0; j != n; ++j) d[i][j] = dot(&vec[i][0], &vec[j][0]);
  upper("D", d, n);
  Kmat kmat(boost::extents[n][n]);
  Gmat gmat(boost::extents[param.size()][n][n]);
#if SK_FEAT_KERNEL == 1
  PolyKernel cm;
  cm.set_degree(std::atoi(argv[2]));
  cm.calculate_matrix(vec, param, kmat, gmat);
#else
  CM::calculate_matrix(vec, param, kmat, gmat);
#endif
  upper("K", kmat, n);
  upper("G0", gmat[0], n);
  if (param.size() > 1) upper("G1", gmat[1], n);
  return 0;
}
