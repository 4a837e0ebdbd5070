// Minimal stand-in for <boost/shared_array.hpp>.  TEST INFRASTRUCTURE ONLY.
// Just enough of boost::shared_array for the reference's optimizer kernels
// (optimizer/rbf_kernel.h: typedef boost::shared_array<svm_node> Data) to
// compile unmodified in tests/cpp/feature_gram_ref_harness.cpp: shared
// ownership of a new[]-allocated array, operator[] and get().  It holds no
// kernel logic.
#ifndef SK_STANDIN_BOOST_SHARED_ARRAY_HPP
#define SK_STANDIN_BOOST_SHARED_ARRAY_HPP

#include <cstddef>
#include <memory>

namespace boost {

template <class T>
class shared_array {
 public:
  typedef T element_type;
  shared_array() {}
  explicit shared_array(T* p) : p_(p, std::default_delete<T[]>()) {}
  T& operator[](std::ptrdiff_t i) const { return p_.get()[i]; }
  T* get() const { return p_.get(); }
  void reset(T* p = 0) { p_.reset(p, std::default_delete<T[]>()); }
  long use_count() const { return p_.use_count(); }

 private:
  std::shared_ptr<T> p_;
};

}  // namespace boost

#endif
