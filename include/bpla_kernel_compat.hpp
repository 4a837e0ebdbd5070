// bpla_kernel_compat.hpp -- drop-in for the BPLA kernel tool (bpla_kernel/):
// replacing
//     #include "data.h"            // bpla's Data<S,IS>, MData, loaders
//     #include "bpla_kernel.h"     // BPLAKernel
// and common/framework.h's  #include "../common/kernel_matrix.h"
// by
//     #include "bpla_kernel_compat.hpp"
// is the only edit; main's code (bpla_kernel/main.cpp:100-127: the score
// table, `LDF ldf;` / `LDF ldf(bp_opts);`, BPLAKernel<double,MData>,
// App<BPLAKernel<double,MData>, LDF>) compiles unchanged and every cell runs
// on the GPU (csrc/kernels/bpla.hip).
//
//   Data<S, IS> / MData = Data<ProfileSequence, list<string>>
//     Data(ma, pf_scale, opts), Data(ma), size()    bpla_kernel/data.h:22-48,
//                                                    data.cpp:19-63
//   DataLoader<MData>(filename, bp_opts, use_bp) / (filename, pf_scales, ...)
//     get()                                          data.h:84-104, data.cpp:181-230
//   DataLoaderFactory<LD>() / (bp_opts)              data.h:136-160
//   BPLAKernel<V, D>(score_table, noBP, SW, gap, ext, alpha, beta)
//     operator()(x, y)                               bpla_kernel.h:13-45
//     static compute_gradients(x, y, score_table, param, d)
//                                                    bpla_kernel.cpp:385-401
//   AAProfileSequence (N_AA, char2aa, size, operator[], n_seqs)
//                                                    common/aaprofile.h:9-77
//   AAMData = Data<AAProfileSequence, list<string>>, DataLoader<AAMData>,
//   DataLoaderFactory<DataLoader<AAMData> >          data.h:52, 118-209
//   BPLAKernel<double,AAMData>(score_table [23][23], noBP = true, ...)
//     the la_kernel tool: the body of la_main.cpp:118-135 compiles with the
//     include swapped and runs on csrc/kernels/la_protein.hip
//   BPMatrix::Options                                common/bpmatrix.h:17-38
//   KernelMatrix<V>                                  common/kernel_matrix.h:13-108
//
// Folding is the engine's McCaskill (notice on stderr; parity against
// ViennaRNA unpinned) unless BPMatrix::Options::fold supplies the bpp.
// `LDF ldf;` (--noBP) builds examples without base pairs: the engine then
// weights every position unpaired (p_left = p_right = 0, p_unpair = 1),
// which the LAScore path never reads.
#ifndef BPLA_KERNEL_COMPAT_HPP
#define BPLA_KERNEL_COMPAT_HPP

#include "skc/core.hpp"

namespace skc {
namespace bpla {

struct BPMatrix {
  typedef BPMatrixOptions Options;
};

struct ProfileSequence {};  // the profile is built by the engine (common/profile.cpp)

// Data<S, IS> (bpla_kernel/data.h:22-48): rows and per-row folded matrices;
// the engine derives the profile and sqrt(p_left / p_right / p_unpair)
// (fill_weight, data.cpp:19-45) when a KernelMatrix needs them.
template <class S, class IS>
struct Data : RowsData {
  typedef S Seq;
  Data() {}
  Data(const IS& ma, float /*pf_scale*/, const BPMatrix::Options& opts) {
    rows.assign(ma.begin(), ma.end());
    use_bp = true;
    fold_rows(*this, opts);
  }
  explicit Data(const IS& ma) { rows.assign(ma.begin(), ma.end()); }
  uint size() const { return rows.empty() ? 0u : (uint)rows.front().size(); }
};

typedef Data<ProfileSequence, std::list<std::string>> MData;

// AAProfileSequence (common/aaprofile.h:9-77, aaprofile.cpp:13-60): the
// integer count of every amino-acid letter per alignment column, everything
// else in slot N_AA.  Host-side view for callers; the engine builds its own
// from the rows (sk_dataset_add_protein).
class AAProfileSequence {
 public:
  typedef float value_type;
  typedef std::vector<value_type> Column;
  typedef std::vector<Column>::const_iterator const_iterator;
  static const unsigned int N_AA = 23;
  static int char2aa(int c) { return sk_char2aa(c); }

  AAProfileSequence() : n_seqs_(0) {}
  template <class T>
  AAProfileSequence(const T& ma) : n_seqs_(0) {
    profile_.assign(ma.begin()->size(), Column(N_AA + 1, 0.0f));
    for (typename T::const_iterator x = ma.begin(); x != ma.end(); ++x) add_sequence(*x);
  }
  value_type n_seqs() const { return n_seqs_; }
  unsigned int size() const { return (unsigned int)profile_.size(); }
  const Column& operator[](unsigned int i) const { return profile_[i]; }
  const_iterator begin() const { return profile_.begin(); }
  const_iterator end() const { return profile_.end(); }
  void add_sequence(const std::string& seq, value_type w = 1.0f) {
    if (profile_.size() != seq.size()) throw "alignment error";
    for (size_t i = 0; i != profile_.size(); ++i) profile_[i][char2aa((unsigned char)seq[i])] += w;
    n_seqs_ += w;
  }

 private:
  value_type n_seqs_;
  std::vector<Column> profile_;
};

// AAMData (bpla_kernel/data.h:52): a protein alignment; Data(ma) only, it
// has no base-pairing weights (data.cpp:51-63).
template <>
struct Data<AAProfileSequence, std::list<std::string>> : RowsData {
  typedef AAProfileSequence Seq;
  Data() {}
  explicit Data(const std::list<std::string>& ma) : seq(ma) { rows.assign(ma.begin(), ma.end()); }
  uint size() const { return seq.size(); }
  AAProfileSequence seq;
};
typedef Data<AAProfileSequence, std::list<std::string>> AAMData;

template <class D>
class DataLoader;

// DataLoader<AAMData> (data.h:118-128, data.cpp:235-293)
template <>
class DataLoader<AAMData> {
 public:
  typedef AAMData Data;
  explicit DataLoader(const char* filename) : file_(filename) {}
  Data* get() {
    std::list<std::string> ma;
    if (!file_.next(ma)) return nullptr;
    for (const std::string& r : ma)
      if (r.size() != ma.front().size()) throw "wrong alignment";  // data.cpp:284-288
    return new AAMData(ma);
  }

 private:
  SeqFile file_;
};

template <>
class DataLoader<MData> {
 public:
  typedef MData Data;
  DataLoader(const char* filename, const BPMatrix::Options& bp_opts, bool use_bp)
      : file_(filename), opts_(bp_opts), use_bp_(use_bp) {}
  DataLoader(const char* filename, const char* /*pf_scales*/, const BPMatrix::Options& bp_opts, bool use_bp)
      : file_(filename), opts_(bp_opts), use_bp_(use_bp) {}
  Data* get() {
    std::list<std::string> ma;
    if (!file_.next(ma)) return nullptr;
    return use_bp_ ? new MData(ma, -1.0f, opts_) : new MData(ma);
  }

 private:
  SeqFile file_;
  BPMatrix::Options opts_;
  bool use_bp_;
};

template <class LD>
class DataLoaderFactory {
 public:
  typedef LD Loader;
  typedef typename Loader::Data Data;
  explicit DataLoaderFactory(const BPMatrix::Options& bp_opts) : bp_opts_(bp_opts), use_bp_(true) {}
  DataLoaderFactory() : use_bp_(false) {}
  Loader* get_loader(const char* filename) const { return new Loader(filename, bp_opts_, use_bp_); }
  Loader* get_loader(const char* filename, const char* pf_scales) const {
    return new Loader(filename, pf_scales, bp_opts_, use_bp_);
  }

 private:
  BPMatrix::Options bp_opts_;
  bool use_bp_;
};

// DataLoaderFactory<DataLoader<AAMData> > (data.h:193-209)
template <>
class DataLoaderFactory<DataLoader<AAMData>> {
 public:
  typedef DataLoader<AAMData> Loader;
  typedef Loader::Data Data;
  DataLoaderFactory() {}
  Loader* get_loader(const char* filename, const char* /*pf_scales*/ = nullptr) const { return new Loader(filename); }
};

template <class ValueType, class DataT>
class BPLAKernel : public KernelBase<ValueType, DataT> {
 public:
  typedef ValueType value_type;
  typedef DataT Data;

  // score_table: any [4][4]-indexable table (the reference passes
  // boost::multi_array<value_type,2>)
  template <class Table>
  BPLAKernel(const Table& score_table, bool noBP, bool SW = false, value_type gap = 1, value_type ext = 1,
             value_type alpha = 1, value_type beta = 1)
      : KernelBase<ValueType, DataT>(noBP ? (SW ? SK_LA_SW : SK_LA) : (SW ? SK_BPLA_SW : SK_BPLA)) {
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b) this->p_.score_table[4 * a + b] = score_table[a][b];
    this->p_.gap = gap;
    this->p_.ext = ext;
    this->p_.alpha = alpha;
    this->p_.beta = beta;
  }

  // the bpla_optimizer's per-pair step: value, d = d/d(alpha, beta, gap,
  // ext) for param = {alpha, beta, gap, ext} (sk_bpla_gradients)
  template <class Table>
  static value_type compute_gradients(const Data& x, const Data& y, const Table& score_table,
                                      const std::vector<double>& param, std::vector<double>& d) {
    sk_kernel_params p;
    sk_kernel_params_default(&p, SK_BPLA);
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b) p.score_table[4 * a + b] = score_table[a][b];
    p.alpha = param.at(0);
    p.beta = param.at(1);
    p.gap = param.at(2);
    p.ext = param.at(3);
    std::vector<std::pair<std::string, Data>> ex{{"+1", x}, {"+1", y}};
    Engine& E = Engine::get();
    const Engine::DsPtr hold = E.dataset(ex, BuildSpec());
    sk_dataset* ds = hold.get();
    const int32_t a = 0, b = 1;
    double v = 0.0, g[4];
    check(sk_bpla_gradients(E.ctx(), ds, ds, &p, &a, &b, 1, &v, g), E.ctx());
    d.assign(g, g + 4);
    return (value_type)v;
  }
};

// BPLAKernel<V, AAMData> (bpla_kernel.cpp:406; la_main.cpp:133): LAScore over
// a [23][23] table in char2aa order.  noBP must be true: AAMData(ma) carries
// no base-pairing weights for BPLAScore to read.
template <class ValueType>
class BPLAKernel<ValueType, AAMData> : public KernelBase<ValueType, AAMData> {
 public:
  typedef ValueType value_type;
  typedef AAMData Data;
  template <class Table>
  BPLAKernel(const Table& score_table, bool noBP, bool SW = false, value_type gap = 1, value_type ext = 1,
             value_type /*alpha*/ = 1, value_type beta = 1)
      : KernelBase<ValueType, AAMData>(SW ? SK_AA_LA_SW : SK_AA_LA) {
    if (!noBP) throw "BPLAKernel<AAMData>: noBP must be true (protein examples have no base-pairing weights)";
    for (int a = 0; a < 23; ++a)
      for (int b = 0; b < 23; ++b) this->p_.aa_score_table[23 * a + b] = score_table[a][b];
    this->p_.gap = gap;
    this->p_.ext = ext;
    this->p_.beta = beta;
  }
};

}  // namespace bpla

template <>
struct ExampleTraits<bpla::AAMData> {
  static void add(sk_dataset* ds, const std::string& label, const bpla::AAMData& d, const BuildSpec&) {
    std::vector<const char*> r;
    for (const auto& s : d.rows) r.push_back(s.c_str());
    check(sk_dataset_add_protein(ds, label.c_str(), (int)r.size(), r.data()));
  }
  static void mix(Fnv& f, const bpla::AAMData& d) {
    mix_rows(f, d);
    f("aa", 2);  // never the cached dataset of the same rows read as RNA
  }
};

template <class S, class IS>
struct ExampleTraits<bpla::Data<S, IS>> {
  static void add(sk_dataset* ds, const std::string& label, const bpla::Data<S, IS>& d, const BuildSpec&) {
    add_rows(ds, label, d, 1.0f);  // th = 1: no DAG (BPLA reads profiles and weights only)
  }
  static void mix(Fnv& f, const bpla::Data<S, IS>& d) { mix_rows(f, d); }
};

}  // namespace skc

#ifndef SKC_NO_REFERENCE_NAMES
using skc::KernelMatrix;
using skc::bpla::BPLAKernel;
using skc::bpla::BPMatrix;
using skc::bpla::Data;
using skc::bpla::DataLoader;
using skc::bpla::DataLoaderFactory;
using skc::bpla::AAMData;
using skc::bpla::AAProfileSequence;
using skc::bpla::MData;
using skc::bpla::ProfileSequence;
typedef unsigned int uint;
#endif

#endif  // BPLA_KERNEL_COMPAT_HPP
