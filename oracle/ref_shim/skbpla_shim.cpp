// Harness for oracle/_ref/libskref_bpla.so: the reference's own, unmodified
//   bpla_kernel/{bpla_kernel,data}.cpp, common/{rna,profile,aaprofile}.cpp
// compiled in place by oracle/Makefile against the stand-in headers, behind a
// C ABI.  Examples are built by the reference's own
// Data(seq, pf_scale, opts) constructor (fill_weight of bpla_kernel/data.cpp)
// on top of the injected BPMatrix of bpmatrix_seam.hpp; the averaged
// base-pairing table is passed in by the caller (see that header).
#include <cstring>
#include <list>
#include <string>
#include <vector>
#include "bpla_kernel.h"
#include "../common/fa.h"
#include "../common/aln.h"
#include "../common/maf.h"
#include "bpmatrix_seam.hpp"

// File loaders (Boost.Spirit in the reference) are named by data.cpp's
// DataLoader::get(), which this library never calls.
typedef BOOST_SPIRIT_CLASSIC_NS::file_iterator<> file_it;
template <> bool load_fa(std::list<std::string>&, file_it&) { return false; }
template <> bool load_aln(std::list<std::string>&, file_it&) { return false; }
template <> bool load_maf(std::list<std::string>&, file_it&) { return false; }

namespace {
boost::multi_array<double, 2> table_of(const double* t16) {
  boost::multi_array<double, 2> t(boost::extents[4][4]);
  for (int a = 0; a != 4; ++a)
    for (int b = 0; b != 4; ++b) t[a][b] = t16[a * 4 + b];
  return t;
}
}  // namespace

extern "C" {

void* skb_data_new(int n_rows, const char* const* rows, const double* avg_packed, int use_bp) {
  std::list<std::string> ma;
  for (int r = 0; r != n_rows; ++r) ma.push_back(std::string(rows[r]));
  if (!use_bp) return new MData(ma);
  BPMatrix::Options opts;
  g_inj = Injected();
  g_inj.avg = avg_packed;
  MData* d = new MData(ma, -1.0f, opts);
  g_inj = Injected();
  return d;
}

void skb_data_free(void* h) { delete static_cast<MData*>(h); }

int skb_seq_len(const void* h) { return (int)static_cast<const MData*>(h)->size(); }

void skb_weights(const void* h, float* p_left, float* p_right, float* p_unpair) {
  const MData& d = *static_cast<const MData*>(h);
  std::copy(d.p_left.begin(), d.p_left.end(), p_left);
  std::copy(d.p_right.begin(), d.p_right.end(), p_right);
  std::copy(d.p_unpair.begin(), d.p_unpair.end(), p_unpair);
}

// BPLAKernel::operator(): exp (sw = 0) or Smith-Waterman (sw = 1) mode, with
// (no_bp = 0) or without the base-pairing score.
double skb_kernel(const void* hx, const void* hy, int no_bp, int sw, double gap, double ext,
                  double alpha, double beta, const double* table16) {
  const boost::multi_array<double, 2> t = table_of(table16);
  BPLAKernel<double, MData> k(t, no_bp != 0, sw != 0, gap, ext, alpha, beta);
  return k(*static_cast<const MData*>(hx), *static_cast<const MData*>(hy));
}

// BPLAKernel::compute_gradients: value and d/d(alpha, beta, gap, ext).
double skb_gradients(const void* hx, const void* hy, double alpha, double beta, double gap,
                     double ext, const double* table16, double* d4) {
  const boost::multi_array<double, 2> t = table_of(table16);
  std::vector<double> param(4), d(4, 0.0);
  param[0] = alpha;
  param[1] = beta;
  param[2] = gap;
  param[3] = ext;
  const double v = BPLAKernel<double, MData>::compute_gradients(
      *static_cast<const MData*>(hx), *static_cast<const MData*>(hy), t, param, d);
  std::copy(d.begin(), d.end(), d4);
  return v;
}
}
