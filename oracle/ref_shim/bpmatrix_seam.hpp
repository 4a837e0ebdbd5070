// The seam shared by the lite and BPLA harnesses: BPMatrix's constructors
// (declared in the reference's common/bpmatrix.h; its common/bpmatrix.cpp,
// which calls ViennaRNA, is not compiled).  The table, the per-row matrices
// and the index maps are filled from arrays the caller injects; the averaging
// of per-row matrices that bpmatrix.cpp does is therefore NOT exercised.
// Included by exactly one translation unit per library.
#ifndef SKREF_BPMATRIX_SEAM_HPP
#define SKREF_BPMATRIX_SEAM_HPP
#include <algorithm>
#include <cctype>
#include <list>
#include <string>
#include <vector>
#include "../common/bpmatrix.h"

namespace {
// Probabilities in flight for the BPMatrix constructors below (set by
// skl_data_new for the duration of one Data constructor).
struct Injected {
  int n_rows;
  const double* const* rows;  // per row, after erase_gap: strict upper, packed
  const double* avg;          // over the aligned length: strict upper, packed
  const double* cur;          // the row whose BPMatrix(string) is being built
} g_inj = {0, 0, 0, 0};

inline size_t packed(size_t i, size_t j, size_t n) { return i * n - i * (i + 1) / 2 + (j - i - 1); }

void fill(BPMatrix& bp, const double* p) {
  const size_t n = bp.size();
  if (!p) return;
  for (size_t i = 0; i != n; ++i)
    for (size_t j = i + 1; j != n; ++j) bp(i + 1, j + 1) = p[packed(i, j, n)];
}
}  // namespace

// ---- the seam: BPMatrix constructors (declared in common/bpmatrix.h) ----
BPMatrix::BPMatrix(const std::string& s, float, const Options&) : sz_(s.size()), table_(sz_ + 1) {
  table_.fill(0.0);
  fill(*this, g_inj.cur);
}

BPMatrix::BPMatrix(const std::string& s, const Options&) : sz_(s.size()), table_(sz_ + 1) {
  table_.fill(0.0);
  fill(*this, g_inj.cur);
}

BPMatrix::BPMatrix(const std::list<std::string>& ma, float pf_scale, const Options& opts)
    : sz_(ma.begin()->size()), table_(sz_ + 1) {
  table_.fill(0.0);
  fill(*this, g_inj.avg);
  int r = 0;
  for (std::list<std::string>::const_iterator x = ma.begin(); x != ma.end(); ++x, ++r) {
    std::string s(*x);
    std::transform(s.begin(), s.end(), s.begin(), ::tolower);
    std::vector<uint> idxmap(s.size(), static_cast<uint>(-1));
    for (uint i = 0, j = 0; i != s.size(); ++i)
      if (s[i] != RNASymbol<char>::GAP) idxmap[i] = j++;
    g_inj.cur = r < g_inj.n_rows ? g_inj.rows[r] : 0;
    boost::shared_ptr<BPMatrix> b(new BPMatrix(erase_gap(s), pf_scale, opts));
    g_inj.cur = 0;
    add_matrix(b, idxmap);
  }
}

BPMatrix::BPMatrix(const std::list<std::string>& ma, const Options& opts)
    : BPMatrix(ma, -1.0f, opts) {}

#endif
