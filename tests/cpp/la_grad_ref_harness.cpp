// Harness of tools/make_golden_la_grad.py and tests/test_la_protein_grad_cpu.py:
// the reference's own BPLAKernel<double,AAMData>::compute_gradients
// (bpla_kernel/bpla_kernel.cpp:385-401, instantiated at :406) over AAMData(ma)
// examples, compiled in place from the reference checkout into a temporary
// directory (nothing compiled from it is kept), with la_ref_harness.cpp's
// compile line:
//
//   g++ -O2 -std=gnu++11 -ffp-contract=off -w -include algorithm
//       -I oracle/ref_shim/standin -I oracle/ref_shim -I $REF/bpla_kernel
//       tests/cpp/la_grad_ref_harness.cpp $REF/bpla_kernel/{bpla_kernel,data}.cpp
//       $REF/common/{rna,profile,aaprofile}.cpp
//
// AAMData(ma) leaves p_left, p_right and p_unpair empty (data.cpp:290), which
// compute_gradients reads: they are filled here with 0, 0, 1 per column, what
// the noBP kernel scores.  alpha = 1.
//
// Input (argv[1], text): la_ref_harness.cpp's format.  Output: per parameter
// set, per x, per y, one line "value d_alpha d_beta d_gap d_ext" of C99 hex
// floats.
#include <cstdio>
#include <list>
#include <string>
#include <vector>
#include "bpla_kernel.h"
#include "../common/fa.h"
#include "../common/aln.h"
#include "../common/maf.h"
#include "bpmatrix_seam.hpp"

// File loaders (Boost.Spirit in the reference) are named by data.cpp's
// DataLoader::get(), which this program never calls.
typedef BOOST_SPIRIT_CLASSIC_NS::file_iterator<> file_it;
template <> bool load_fa(std::list<std::string>&, file_it&) { return false; }
template <> bool load_aln(std::list<std::string>&, file_it&) { return false; }
template <> bool load_maf(std::list<std::string>&, file_it&) { return false; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_ex = 0;
  if (std::fscanf(f, "%d", &n_ex) != 1) return 2;
  std::vector<AAMData*> ex;
  char buf[1 << 16];
  for (int e = 0; e < n_ex; ++e) {
    int n_rows = 0;
    if (std::fscanf(f, "%d", &n_rows) != 1) return 2;
    std::list<std::string> ma;
    for (int r = 0; r < n_rows; ++r) {
      if (std::fscanf(f, "%65535s", buf) != 1) return 2;
      ma.push_back(std::string(buf));
    }
    AAMData* d = new AAMData(ma);
    d->p_left.assign(d->size(), 0.0f);
    d->p_right.assign(d->size(), 0.0f);
    d->p_unpair.assign(d->size(), 1.0f);
    ex.push_back(d);
  }
  int n_par = 0;
  if (std::fscanf(f, "%d", &n_par) != 1) return 2;
  for (int p = 0; p < n_par; ++p) {
    double gap, ext, beta;
    if (std::fscanf(f, "%lf %lf %lf", &gap, &ext, &beta) != 3) return 2;
    boost::multi_array<double, 2> t(boost::extents[23][23]);
    for (int a = 0; a < 23; ++a)
      for (int b = 0; b < 23; ++b)
        if (std::fscanf(f, "%lf", &t[a][b]) != 1) return 2;
    std::vector<double> param(4), d(4);
    param[0] = 1.0;
    param[1] = beta;
    param[2] = gap;
    param[3] = ext;
    for (int x = 0; x < n_ex; ++x)
      for (int y = 0; y < n_ex; ++y) {
        const double v = BPLAKernel<double, AAMData>::compute_gradients(*ex[x], *ex[y], t, param, d);
        std::printf("%a %a %a %a %a\n", v, d[0], d[1], d[2], d[3]);
      }
  }
  std::fclose(f);
  return 0;
}
