// Harness of tools/make_golden_la.py and tests/test_la_protein_cpu.py: the
// reference's own BPLAKernel<double,AAMData> (bpla_kernel/bpla_kernel.cpp:406)
// over AAMData(ma) examples, compiled in place from the reference checkout
// into a temporary directory (nothing compiled from it is kept):
//
//   g++ -O2 -std=gnu++11 -ffp-contract=off -w -include algorithm
//       -I oracle/ref_shim/standin -I oracle/ref_shim -I $REF/bpla_kernel
//       tests/cpp/la_ref_harness.cpp $REF/bpla_kernel/{bpla_kernel,data}.cpp
//       $REF/common/{rna,profile,aaprofile}.cpp
//
// Input (argv[1], text): the example count; per example its row count and
// rows; the parameter-set count; per set gap, ext, beta and the 23x23 table
// (529 numbers, [x residue][y residue]).  Output: per parameter set, per mode
// (exp, then SW), per x, per y, K(x, y) as a C99 hex float, one per line.
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
    ex.push_back(new AAMData(ma));
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
    for (int sw = 0; sw < 2; ++sw) {
      BPLAKernel<double, AAMData> k(t, true, sw != 0, gap, ext, 1.0, beta);
      for (int x = 0; x < n_ex; ++x)
        for (int y = 0; y < n_ex; ++y) std::printf("%a\n", k(*ex[x], *ex[y]));
    }
  }
  std::fclose(f);
  return 0;
}
