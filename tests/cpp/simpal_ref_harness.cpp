// Harness of tools/make_golden_simpal.py and tests/test_simpal_cpu.py: the
// reference's own Pals and KernelFunc (simpal/simpal.cpp:30-280), compiled in
// place from the reference checkout into a temporary directory (nothing
// compiled from it is kept):
//
//   g++ -O2 -std=gnu++11 -ffp-contract=off -w -I tests/cpp/simpal_standin
//       -I oracle/ref_shim/standin -I $REF/simpal tests/cpp/simpal_ref_harness.cpp
//
// The reference's file is included whole, its main renamed; KernelMatrix is a
// dummy (its header's guard is defined here), the Fasta members are stubs,
// and PFWrapper::fold, which calls ViennaRNA in the reference, is the seam:
// it fills pr_ / iindx_ from the injected base-pairing probabilities with
// ViennaRNA's index iindx[i] = ((n + 1 - i)(n - i)) / 2 + n + 1.
//
// Input (argv[1], text): the example count; per example its sequence,
// seed_length, min_loop, max_dist and the n(n-1)/2 probabilities (packed
// strict upper triangle, row-major); the query count; per query x, y and the
// tolerance.  The sequence is lowercased here, as load_examples does (:298).
// Output: per example "E <entries>" and per entry "<key> <dist> <weight>", in
// map order; per query K(x, y); values as C99 hex floats.
#include <cassert>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include <ext/hash_map>

#define __INC_KERNEL_MATRIX_H__
template <class V>
struct KernelMatrix {
  template <class E, class K>
  void calculate(const E&, const K&, bool, unsigned) {}
  template <class E, class K>
  void calculate(const E&, const E&, const K&, bool, bool, unsigned) {}
  void print(std::ostream&) const {}
  V operator()(unsigned) const { return V(); }
};

// the map of a Pals is private: the harness prints it
#define private public
#define main simpal_reference_main
#include "simpal.cpp"
#undef main
#undef private

static const double* g_bpp = 0;

float PFWrapper::fold(std::string&) {
  const int n = (int)seq_.size();
  for (int i = 0; i <= n; ++i) iindx_[i] = ((n + 1 - i) * (n - i)) / 2 + n + 1;
  for (size_t k = 0; k < pr_.size(); ++k) pr_[k] = 0.0;
  size_t k = 0;
  for (int i = 1; i <= n; ++i)
    for (int j = i + 1; j <= n; ++j) pr_[iindx_[i] - j] = g_bpp[k++];
  return 0.0f;
}

Fasta::Fasta(std::istream& istrm) : m_istrm(istrm) {}
Fasta::~Fasta() {}
const char* Fasta::GetNextSeq() { return 0; }
void Fasta::ToUpper() {}
void Fasta::ToLower() {}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_ex = 0;
  if (std::fscanf(f, "%d", &n_ex) != 1) return 2;
  std::vector<Pals> ex;
  static char buf[1 << 16];
  for (int e = 0; e < n_ex; ++e) {
    unsigned s = 0, min_loop = 0, max_dist = 0;
    if (std::fscanf(f, "%65535s %u %u %u", buf, &s, &min_loop, &max_dist) != 4) return 2;
    std::string seq(buf);
    for (size_t k = 0; k < seq.size(); ++k) seq[k] = (char)std::tolower((unsigned char)seq[k]);
    const size_t n = seq.size();
    std::vector<double> bpp(n * (n - 1) / 2 + 1);
    for (size_t k = 0; k < n * (n - 1) / 2; ++k)
      if (std::fscanf(f, "%lf", &bpp[k]) != 1) return 2;
    g_bpp = bpp.data();
    std::cout.setstate(std::ios_base::failbit);  // the "m\tn" lines of :169
    ex.push_back(Pals(seq, s, min_loop, max_dist));
    std::cout.clear();
    const Pals& P = ex.back();
    std::printf("E %u\n", (unsigned)P.pals_.size());
    for (Pals::PalMap::const_iterator it = P.pals_.begin(); it != P.pals_.end(); ++it)
      std::printf("%s %d %a\n", it->first.key_.c_str(), it->first.dist_, (double)it->second);
  }
  int n_q = 0;
  if (std::fscanf(f, "%d", &n_q) != 1) return 2;
  for (int q = 0; q < n_q; ++q) {
    int x, y, tol;
    if (std::fscanf(f, "%d %d %d", &x, &y, &tol) != 3) return 2;
    if (x < 0 || x >= n_ex || y < 0 || y >= n_ex) return 2;
    std::printf("%a\n", KernelFunc(tol)(ex[x], ex[y]));
  }
  std::fclose(f);
  return 0;
}
