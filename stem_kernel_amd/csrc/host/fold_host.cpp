// Host pieces of the GPU folds: see fold_host.h.
#include "host/fold_host.h"

#include <algorithm>
#include <cmath>

#include "host/fold_params.h"
#include "kernels/fold_ali_model.h"

namespace sk {

// Laid out in one buffer: the fixed-size tables first (o_st .. o_ml, n_small
// doubles), then the two whose length follows the batch's longest sequence
// max_len (hairpin, scale powers), so a launch whose tables outgrow the LDS
// keeps the first part in LDS and reads the tail from HBM (fold.hip GTAB).
// Entry k of every table is the same double whatever max_len is.
void fold_tables(int max_len, FoldLaunch& L, std::vector<double>& t) {
  using namespace foldp;
  t.clear();
  auto bz = [](double e) { return std::exp(-e / kT); };
  L.o_st = (int32_t)t.size();
  for (int a = 0; a < 7; ++a)
    for (int b = 0; b < 7; ++b) t.push_back(a && b ? bz(stack37[a][b]) : 0.0);
  L.o_bu = (int32_t)t.size();
  for (int k = 0; k <= max_loop; ++k) t.push_back(k ? bz(bulge37[k]) : 0.0);
  L.o_in = (int32_t)t.size();
  for (int k = 0; k <= max_loop; ++k) t.push_back(k >= 2 ? bz(interior37[k]) : 0.0);
  L.o_ni = (int32_t)t.size();
  for (int k = 0; k <= max_loop; ++k) t.push_back(bz(std::min(max_ninio, ninio * k)));
  L.o_au = (int32_t)t.size();
  for (int k = 0; k < 7; ++k) t.push_back(k > 2 ? bz(terminal_au) : 1.0);
  L.o_ml = (int32_t)t.size();
  t.push_back(bz(ml_closing + ml_intern));
  t.push_back(bz(ml_intern));
  L.n_small = (int32_t)t.size();
  L.o_hp = (int32_t)t.size();
  for (int k = 0; k <= max_len + 1; ++k) {
    if (k < 3) {
      t.push_back(0.0);
      continue;
    }
    double e = hairpin37[k <= 30 ? k : 30];
    if (k > 30) e += lxc * std::log((double)k / 30.0);
    t.push_back(bz(e));
  }
  L.o_scp = (int32_t)t.size();
  for (int k = 0; k <= max_len + 2; ++k) t.push_back(std::exp(log_sc * k));
  L.log_sc = log_sc;
  L.n_tab = (int32_t)t.size();
  L.n_tab_pad = (L.n_tab + 1) & ~1;
}

void fold_tables_ali(FoldLaunch& L, std::vector<double>& t) {
  L.o_ali = (int32_t)t.size();
  for (int a = 0; a < 8; ++a)
    for (int b = 0; b < 8; ++b)
      t.push_back(a >= 1 && a <= 6 && b >= 1 && b <= 6 ? (double)foldp::stack37[a][b] : 0.0);
  t.push_back(foldp::kT);
  t.push_back((double)foldp::terminal_au);
  t.push_back((double)foldp::bulge37[1]);
  L.n_tab = (int32_t)t.size();
  L.n_tab_pad = (L.n_tab + 1) & ~1;
}

static int8_t fold_code(char ch) {
  switch (ch) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'U': case 'u': case 'T': case 't': return 3;
    default: return -1;
  }
}

void fold_codes(const char* s, size_t n, int8_t* out) {
  for (size_t a = 0; a < n; ++a) out[a] = fold_code(s[a]);
}

// --noLonelyPairs (common/bpmatrix.cpp:56-58, 149, Vienna::noLonelyPairs):
// the legacy ViennaRNA partition function applies it through its pair-type
// table only (1.8 part_func.c make_ptypes; not vendored).  Walking each chain
// (i, j), (i-1, j+1), ... outward from its innermost pair (j - i = 4 or 5),
// a pair is dropped when its inner neighbour was dropped or cannot pair and
// its outer neighbour cannot pair; the outer type is re-read only inside the
// sequence, so a chain's outermost pair compares against its own type.
// (can(i, j): whether the pair can form at all; codes: fold_code, -1 never
// pairs)
template <class Can>
static void lonely_pair_walk(int n, Can can, uint8_t* lp) {
  std::fill(lp, lp + (size_t)n * n, (uint8_t)0);
  for (int k = 0; k < n; ++k)
    for (int l = 1; l <= 2; ++l) {
      int i = k, j = k + 3 + l, otype = 0, ntype = 0;
      if (j >= n) continue;
      int type = can(i, j);
      for (; i >= 0 && j < n; --i, ++j) {
        if (i > 0 && j < n - 1) ntype = can(i - 1, j + 1);
        if (!otype && !ntype) type = 0;
        lp[(size_t)i * n + j] = type != 0;
        otype = type;
        type = ntype;
      }
    }
}

void lonely_pair_table(const int8_t* c, int n, bool no_gu, uint8_t* lp) {
  lonely_pair_walk(n, [&](int i, int j) {
    const int t = ali_row_type(c[i], c[j], no_gu);  // (7: neither is a nucleotide)
    return t == 7 ? 0 : t;
  }, lp);
}

void lonely_pair_table_ali(const int8_t* c, int n_rows, int n, bool no_gu, uint8_t* lp) {
  std::vector<uint8_t> ok((size_t)n * n, 0);
  for (int i = 0; i < n; ++i)
    for (int j = i + 4; j < n; ++j) {
      AliCounts pf;
      for (int s = 0; s < n_rows; ++s) pf.add(ali_row_type(c[(size_t)s * n + i], c[(size_t)s * n + j], no_gu));
      int64_t ps = 0;
      ok[(size_t)i * n + j] = ali_allowed(pf, n_rows, j - i, &ps);
    }
  lonely_pair_walk(n, [&](int i, int j) { return (int)ok[(size_t)i * n + j]; }, lp);
}

int32_t fold_batch_end(int32_t b0, int32_t n, double budget, const std::function<double(int32_t)>& bytes) {
  double sum = 0.0;
  int32_t b1 = b0;
  for (; b1 < n; ++b1) {
    const double w = bytes(b1);
    if (b1 > b0 && sum + w > budget) break;
    sum += w;
  }
  return b1;
}

}  // namespace sk
