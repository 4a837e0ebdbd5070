// Harness for oracle/_ref/libskref_lite.so: the reference's own, unmodified
//   stem_kernel_lite/{data,stem_kernel,score_table,string_kernel,ribosum}.cpp
//   common/{rna,profile}.cpp
// compiled in place by oracle/Makefile against the stand-in headers of
// oracle/ref_shim/standin/, behind a C ABI (tests/test_oracle_dp_pinning.py).
//
// ViennaRNA is not available, so base-pairing probabilities enter where the
// product takes them too: this file defines BPMatrix's constructors (the
// reference's common/bpmatrix.cpp is not compiled) and fills the table, the
// per-row matrices and the index maps from arrays the caller passes in.
// Everything downstream -- Profiler, DAGBuilder, find_root, find_max_parent,
// fill_weight and every kernel -- is the reference's own code.
// The averaging of per-row matrices into the alignment's matrix lives in
// bpmatrix.cpp next to the ViennaRNA calls and so stays unpinned: the caller
// passes the averaged table in.
#include <algorithm>
#include <cctype>
#include <cstring>
#include <list>
#include <string>
#include <vector>
#include "data.h"
#include "def_kernel.h"
#include "../common/fa.h"
#include "../common/aln.h"
#include "../common/maf.h"
#include "bpmatrix_seam.hpp"

// The file loaders of common/{fa,aln,maf}.cpp need Boost.Spirit; data.cpp only
// names them from DataLoader<MData>::get(), which this library never calls.
typedef BOOST_SPIRIT_CLASSIC_NS::file_iterator<> file_it;
template <> bool load_fa(std::list<std::string>&, file_it&) { return false; }
template <> bool load_aln(std::list<std::string>&, file_it&) { return false; }
template <> bool load_maf(std::list<std::string>&, file_it&) { return false; }

extern "C" {

// One example through the reference's Data(seq, th, pf_scale, opts)
// constructor (use_bp) or Data(seq) (no DAG, empty weight).
void* skl_data_new(int n_rows, const char* const* rows, const double* const* bpp_rows,
                   const double* avg_packed, float th, int use_bp) {
  std::list<std::string> ma;
  for (int r = 0; r != n_rows; ++r) ma.push_back(std::string(rows[r]));
  if (!use_bp) return new MData(ma);
  BPMatrix::Options opts;
  g_inj.n_rows = n_rows;
  g_inj.rows = bpp_rows;
  g_inj.avg = avg_packed;
  g_inj.cur = 0;
  MData* d = new MData(ma, th, -1.0f, opts);
  g_inj = Injected();
  return d;
}

void skl_data_free(void* h) { delete static_cast<MData*>(h); }

int skl_n_nodes(const void* h) { return (int)static_cast<const MData*>(h)->tree.size(); }
int skl_seq_len(const void* h) { return (int)static_cast<const MData*>(h)->seq.size(); }
int skl_n_weight(const void* h) { return (int)static_cast<const MData*>(h)->weight.size(); }
int skl_n_roots(const void* h) { return (int)static_cast<const MData*>(h)->root.size(); }
int skl_n_edges(const void* h) {
  const MData& d = *static_cast<const MData*>(h);
  size_t n = 0;
  for (size_t i = 0; i != d.tree.size(); ++i) n += d.tree[i].size();
  return (int)n;
}
int skl_n_bpfreq(const void* h) {
  const MData& d = *static_cast<const MData*>(h);
  size_t n = 0;
  for (size_t i = 0; i != d.tree.size(); ++i)
    n += std::distance(d.tree[i].bp_freq_begin(), d.tree[i].bp_freq_end());
  return (int)n;
}

void skl_nodes(const void* h, unsigned* first, unsigned* last, unsigned* n_edges,
               unsigned* n_bpfreq, float* weight, unsigned* max_pa) {
  const MData& d = *static_cast<const MData*>(h);
  for (size_t i = 0; i != d.tree.size(); ++i) {
    first[i] = d.tree[i].first();
    last[i] = d.tree[i].last();
    n_edges[i] = d.tree[i].size();
    n_bpfreq[i] = std::distance(d.tree[i].bp_freq_begin(), d.tree[i].bp_freq_end());
    weight[i] = d.tree[i].weight();
    max_pa[i] = d.max_pa[i];
  }
}

void skl_edges(const void* h, unsigned* to, unsigned* gaps) {
  const MData& d = *static_cast<const MData*>(h);
  size_t k = 0;
  for (size_t i = 0; i != d.tree.size(); ++i)
    for (MData::Node::const_iterator e = d.tree[i].begin(); e != d.tree[i].end(); ++e, ++k) {
      to[k] = e->to();
      gaps[k] = e->gaps();
    }
}

void skl_bpfreq(const void* h, unsigned* code, float* p) {
  const MData& d = *static_cast<const MData*>(h);
  size_t k = 0;
  for (size_t i = 0; i != d.tree.size(); ++i)
    for (DAG::bp_freq_iterator b = d.tree[i].bp_freq_begin(); b != d.tree[i].bp_freq_end();
         ++b, ++k) {
      code[k] = b->first.first * 4u + b->first.second;
      p[k] = b->second;
    }
}

void skl_roots(const void* h, unsigned* roots) {
  const MData& d = *static_cast<const MData*>(h);
  std::copy(d.root.begin(), d.root.end(), roots);
}

void skl_weight(const void* h, float* w) {
  const MData& d = *static_cast<const MData*>(h);
  std::copy(d.weight.begin(), d.weight.end(), w);
}

// K(x, y) by the reference's kernel classes.  kind: 0 SuStem, 1 SiStem,
// 2 StringKernel(gap, alpha), 3 StringKernel(gap, match, mismatch),
// 4 SuStemStr, 5 SiStemStr, 6 LSuStem, 7 LSuStemStr (def_kernel.h).
// p = {loop_gap, beta, stack, covar, gap, alpha, match, mismatch}
double skl_kernel(int kind, const void* hx, const void* hy, const double* p, unsigned len_band) {
  const MData& x = *static_cast<const MData*>(hx);
  const MData& y = *static_cast<const MData*>(hy);
  const double loop_gap = p[0], beta = p[1], stack = p[2], covar = p[3], gap = p[4], alpha = p[5],
               match = p[6], mismatch = p[7];
  switch (kind) {
    case 0: { SuStemKernel<double, MData> k(loop_gap, beta, len_band); return k(x, y); }
    case 1: { SiStemKernel<double, MData> k(loop_gap, stack, covar, len_band); return k(x, y); }
    case 2: { StringKernel<double, MData> k(gap, alpha); return k(x, y); }
    case 3: { StringKernel<double, MData> k(gap, match, mismatch); return k(x, y); }
    case 4: { SuStemStrKernel<double, MData> k(alpha, beta, loop_gap, gap, len_band); return k(x, y); }
    case 5: {
      SiStemStrKernel<double, MData> k(loop_gap, stack, covar, gap, match, mismatch, len_band);
      return k(x, y);
    }
    case 6: { LSuStemKernel<double, MData> k(loop_gap, beta, len_band); return k(x, y); }
    case 7: { LSuStemStrKernel<double, MData> k(alpha, beta, loop_gap, gap, len_band); return k(x, y); }
  }
  return -1.0;
}
}
