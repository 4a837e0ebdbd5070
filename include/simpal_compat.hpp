// simpal_compat.hpp -- drop-in for the reference's simple palindrome kernel
// tool (simpal/, --enable-simpal): with lines 30-280 of simpal/simpal.cpp
// (class Pals, class KernelFunc) and its includes of ../common/kernel_matrix.h
// and ../common/fasta.h replaced by
//     #include "simpal_compat.hpp"
// the rest of the file (simpal.cpp:282-423: Example / ExampleSet,
// load_examples, main with Fasta, KernelFunc(tolerance), KernelMatrix::
// calculate / print / operator()(i)) compiles against the engine and every
// Gram cell is computed on the GPU (sk_gram / sk_test_matrix over SK_SIMPAL,
// csrc/kernels/simpal.hip).  tests/cpp/simpal_dropin.cpp is such a main.
//
//   Pals(seq, seed_length, min_loop, max_dist)     simpal/simpal.cpp:32-223
//   KernelFunc(tolerance = 1), value_type, operator()(Pals, Pals)   :225-280
//   Fasta                                           common/fasta.h:14-40
//   KernelMatrix<V>                                 common/kernel_matrix.h:13-108
//
// Kept exactly: the map of a sequence and its float weights, the order of the
// kernel's terms' factors, the tolerance semantics (negative: every key pair
// counts), NaN off the diagonal of a zero-diagonal example under -n (see
// sk_dataset_add_palindromes in stem_kernel.h).
// Differs: weights of one (key, d) are added in a defined order (increasing
// i, then r) where the reference follows a hash_multimap's iteration order;
// the "m\tn" lines the reference prints while it builds a map are not
// printed; the reference folds with ViennaRNA (PFWrapper(seq, noGU = true)),
// here each sequence is folded once by the engine's McCaskill without GU
// pairs (notice on stderr; parity against ViennaRNA unpinned) or by
// skc::simpal_fold() when set.  A Pals keeps its sequence and parameters; the
// engine builds the map when a kernel or a KernelMatrix needs it.
#ifndef SIMPAL_COMPAT_HPP
#define SIMPAL_COMPAT_HPP

#include "skc/core.hpp"
#include "skc/example.hpp"

namespace skc {

// fold used for the examples (empty: the engine's GPU McCaskill)
inline FoldFn& simpal_fold() {
  static FoldFn f;
  return f;
}

class Pals {
 public:
  Pals() : seed_length_(0), min_loop_(0), max_dist_(0) {}
  Pals(const std::string& seq, uint seed_length, uint min_loop, uint max_dist)
      : seq_(seq), seed_length_(seed_length), min_loop_(min_loop), max_dist_(max_dist) {}
  const std::string& sequence() const { return seq_; }
  uint seed_length() const { return seed_length_; }
  uint min_loop() const { return min_loop_; }
  uint max_dist() const { return max_dist_; }

 private:
  std::string seq_;
  uint seed_length_, min_loop_, max_dist_;
};

template <>
struct ExampleTraits<Pals> {
  static void add(sk_dataset* ds, const std::string& label, const Pals& p, const BuildSpec& spec) {
    // the loader lowercases (simpal.cpp:298); the fold sees what the builder sees
    std::string seq = p.sequence();
    std::transform(seq.begin(), seq.end(), seq.begin(), [](unsigned char c) { return (char)std::tolower(c); });
    if (p.seed_length() > 32 || p.min_loop() > 0x7fffffffu) throw "palindrome seed_length or min_loop not supported";
    std::vector<std::vector<double>> bpp;
    if (spec.fold_fn) {
      bpp.emplace_back();
      spec.fold_fn(seq, (spec.fold_flags & SK_FOLD_NO_GU) != 0, bpp.back());
    } else {
      Engine::get().fold(std::vector<std::string>(1, seq), spec.fold_flags, bpp);
    }
    // a dist never exceeds the sequence length, so a larger max_dist cuts nothing
    const int32_t md = (int32_t)std::min<uint>(p.max_dist(), 0x7fffffffu);
    check(sk_dataset_add_palindromes(ds, label.c_str(), seq.c_str(), bpp[0].data(), (int32_t)p.seed_length(),
                                     (int32_t)p.min_loop(), md));
  }
  static void mix(Fnv& f, const Pals& p) {
    f(p.sequence().data(), p.sequence().size() + 1);
    const uint v[3] = {p.seed_length(), p.min_loop(), p.max_dist()};
    f(v, sizeof v);
  }
};

class KernelFunc : public KernelBase<double, Pals> {
 public:
  typedef double value_type;

  KernelFunc(int tolerance = 1) : KernelBase<double, Pals>(SK_SIMPAL) {
    this->p_.mismatch = (double)tolerance;
    this->spec_.fold = true;
    this->spec_.fold_flags = SK_FOLD_NO_GU;  // PFWrapper(seq, true), simpal.cpp:128
    this->spec_.fold_fn = simpal_fold();
  }
};

}  // namespace skc

#ifndef SKC_NO_REFERENCE_NAMES
using skc::Fasta;
using skc::KernelFunc;
using skc::KernelMatrix;
using skc::Pals;
typedef unsigned int uint;
#endif

#endif  // SIMPAL_COMPAT_HPP
