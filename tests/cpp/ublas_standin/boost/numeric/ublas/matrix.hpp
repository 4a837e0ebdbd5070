// Minimal stand-in for <boost/numeric/ublas/matrix.hpp>.  TEST INFRASTRUCTURE
// ONLY (see vector.hpp beside it): a dense row-major matrix and
// prod(matrix, vector), which accumulates each row from zero in ascending
// column index, as uBLAS's matrix_vector_prod1 functor does without its
// Duff-device option.
#ifndef SK_UBLAS_STANDIN_MATRIX_HPP
#define SK_UBLAS_STANDIN_MATRIX_HPP

#include "vector.hpp"

namespace boost { namespace numeric { namespace ublas {

template <class T>
class matrix {
 public:
  typedef std::size_t size_type;
  matrix() : r_(0), c_(0) {}
  matrix(size_type r, size_type c) : r_(r), c_(c), d_(r * c) {}
  size_type size1() const { return r_; }
  size_type size2() const { return c_; }
  T& operator()(size_type i, size_type j) { assert(i < r_ && j < c_); return d_[i * c_ + j]; }
  const T& operator()(size_type i, size_type j) const { assert(i < r_ && j < c_); return d_[i * c_ + j]; }

 private:
  size_type r_, c_;
  std::vector<T> d_;
};

template <class T>
vector<T> prod(const matrix<T>& A, const vector<T>& v) {
  assert(A.size2() == v.size());
  ++standin_prod_calls();
  vector<T> r(A.size1());
  for (std::size_t i = 0; i != A.size1(); ++i) {
    T t = T();
    for (std::size_t j = 0; j != A.size2(); ++j) t += A(i, j) * v(j);
    r(i) = t;
  }
  return r;
}

}}}  // namespace boost::numeric::ublas

#endif
