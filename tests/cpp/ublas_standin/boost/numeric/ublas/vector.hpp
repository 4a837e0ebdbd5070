// Minimal stand-in for <boost/numeric/ublas/vector.hpp>.  TEST INFRASTRUCTURE
// ONLY: just enough of uBLAS's dense vector for the reference's
// optimizer/gradient.cpp to compile unmodified (tools/make_golden_auc_gradient.py).
// Expressions are evaluated eagerly, element by element; inner_prod
// accumulates from zero in ascending index, which is what uBLAS's
// vector_inner_prod functor does without its Duff-device option.  Holds no
// logic of the gradient.
#ifndef SK_UBLAS_STANDIN_VECTOR_HPP
#define SK_UBLAS_STANDIN_VECTOR_HPP

#include <cassert>
#include <cstddef>
#include <vector>

namespace boost { namespace numeric { namespace ublas {

// what the harness reads: calls of prod(matrix, vector) so far
inline long& standin_prod_calls() {
  static long n = 0;
  return n;
}

template <class T>
class vector {
 public:
  typedef std::size_t size_type;
  typedef T value_type;
  vector() {}
  explicit vector(size_type n) : d_(n) {}
  vector(size_type n, const T& v) : d_(n, v) {}
  size_type size() const { return d_.size(); }
  void resize(size_type n, bool = true) { d_.resize(n); }
  T& operator()(size_type i) { assert(i < d_.size()); return d_[i]; }
  const T& operator()(size_type i) const { assert(i < d_.size()); return d_[i]; }
  T& operator[](size_type i) { return (*this)(i); }
  const T& operator[](size_type i) const { return (*this)(i); }
  vector& operator+=(const vector& o) {
    assert(o.size() == size());
    for (size_type i = 0; i != size(); ++i) d_[i] += o.d_[i];
    return *this;
  }
  vector& operator-=(const vector& o) {
    assert(o.size() == size());
    for (size_type i = 0; i != size(); ++i) d_[i] -= o.d_[i];
    return *this;
  }

 private:
  std::vector<T> d_;
};

template <class T>
class zero_vector : public vector<T> {
 public:
  explicit zero_vector(std::size_t n) : vector<T>(n, T()) {}
};

template <class T>
vector<T> operator-(const vector<T>& a) {
  vector<T> r(a.size());
  for (std::size_t i = 0; i != a.size(); ++i) r(i) = -a(i);
  return r;
}
template <class T>
vector<T> operator+(const vector<T>& a, const vector<T>& b) {
  assert(a.size() == b.size());
  vector<T> r(a.size());
  for (std::size_t i = 0; i != a.size(); ++i) r(i) = a(i) + b(i);
  return r;
}
template <class T>
vector<T> operator-(const vector<T>& a, const vector<T>& b) {
  assert(a.size() == b.size());
  vector<T> r(a.size());
  for (std::size_t i = 0; i != a.size(); ++i) r(i) = a(i) - b(i);
  return r;
}
template <class T>
vector<T> operator*(const T& s, const vector<T>& a) {
  vector<T> r(a.size());
  for (std::size_t i = 0; i != a.size(); ++i) r(i) = s * a(i);
  return r;
}
template <class T>
T inner_prod(const vector<T>& a, const vector<T>& b) {
  assert(a.size() == b.size());
  T t = T();
  for (std::size_t i = 0; i != a.size(); ++i) t += a(i) * b(i);
  return t;
}

}}}  // namespace boost::numeric::ublas

#endif
