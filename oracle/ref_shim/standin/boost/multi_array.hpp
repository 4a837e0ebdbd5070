// Minimal stand-in for <boost/multi_array.hpp>.  TEST INFRASTRUCTURE ONLY.
// Just enough of the public Boost.MultiArray interface for the reference DP
// sources to compile unmodified (oracle/Makefile): a dense row-major N-d array
// whose elements are value-initialised (zero for arithmetic types), also
// after resize(); operator[] chains through sub-views down to an element
// reference; size() on the array and on a sub-view is the leading extent.
// It holds no DP logic.  Checked by tests/cpp/standin_multi_array.cpp.
#ifndef SKREF_STANDIN_BOOST_MULTI_ARRAY_HPP
#define SKREF_STANDIN_BOOST_MULTI_ARRAY_HPP

#include <algorithm>
#include <cassert>
#include <cstddef>
#include <vector>

namespace boost {

namespace detail { namespace multi_array {

template <std::size_t N>
struct extent_gen {
  std::size_t ext[N ? N : 1];
  extent_gen<N + 1> operator[](std::size_t e) const {
    extent_gen<N + 1> r;
    for (std::size_t k = 0; k != N; ++k) r.ext[k] = ext[k];
    r.ext[N] = e;
    return r;
  }
};

// A view of the trailing N dimensions at a fixed prefix of indices.
template <class T, std::size_t N>
class sub_array {
 public:
  typedef T element;
  typedef std::size_t size_type;
  typedef std::size_t index;
  sub_array(T* base, const size_type* shape, const size_type* strides)
      : base_(base), shape_(shape), strides_(strides) {}
  sub_array<T, N - 1> operator[](index i) const {
    assert(i < shape_[0]);
    return sub_array<T, N - 1>(base_ + i * strides_[0], shape_ + 1, strides_ + 1);
  }
  size_type size() const { return shape_[0]; }
  const size_type* shape() const { return shape_; }
  size_type num_elements() const {
    size_type n = 1;
    for (std::size_t k = 0; k != N; ++k) n *= shape_[k];
    return n;
  }

 private:
  T* base_;
  const size_type* shape_;
  const size_type* strides_;
};

template <class T>
class sub_array<T, 1> {
 public:
  typedef T element;
  typedef std::size_t size_type;
  typedef std::size_t index;
  sub_array(T* base, const size_type* shape, const size_type* strides)
      : base_(base), shape_(shape), strides_(strides) {}
  T& operator[](index i) const {
    assert(i < shape_[0]);
    return base_[i * strides_[0]];
  }
  size_type size() const { return shape_[0]; }
  const size_type* shape() const { return shape_; }
  size_type num_elements() const { return shape_[0]; }

 private:
  T* base_;
  const size_type* shape_;
  const size_type* strides_;
};

template <class T, std::size_t N>
struct sub_of {
  typedef sub_array<T, N - 1> reference;
  static reference get(T* base, const std::size_t* shape, const std::size_t* strides,
                       std::size_t i) {
    assert(i < shape[0]);
    return reference(base + i * strides[0], shape + 1, strides + 1);
  }
};
template <class T>
struct sub_of<T, 1> {
  typedef T& reference;
  static reference get(T* base, const std::size_t* shape, const std::size_t* strides,
                       std::size_t i) {
    assert(i < shape[0]);
    return base[i * strides[0]];
  }
};

}}  // namespace detail::multi_array

static const detail::multi_array::extent_gen<0> extents = detail::multi_array::extent_gen<0>();

template <class T, std::size_t N>
class multi_array {
 public:
  typedef T element;
  typedef std::size_t size_type;
  typedef std::size_t index;
  typedef typename detail::multi_array::sub_of<T, N>::reference reference;
  typedef typename detail::multi_array::sub_of<const T, N>::reference const_reference;
  static const std::size_t dimensionality = N;

  multi_array() : data_() { set_shape(zero_extents()); }
  explicit multi_array(const detail::multi_array::extent_gen<N>& e) : data_() {
    set_shape(e);
    data_.assign(total(), T());
  }

  // Boost semantics: elements inside both the old and the new extents keep
  // their values, every other element is value-initialised.
  void resize(const detail::multi_array::extent_gen<N>& e) {
    multi_array fresh(e);
    size_type common[N];
    bool any = !data_.empty() && !fresh.data_.empty();
    for (std::size_t k = 0; k != N; ++k) {
      common[k] = std::min(shape_[k], fresh.shape_[k]);
      if (common[k] == 0) any = false;
    }
    if (any) {
      size_type idx[N];
      for (std::size_t k = 0; k != N; ++k) idx[k] = 0;
      for (;;) {
        size_type from = 0, to = 0;
        for (std::size_t k = 0; k != N; ++k) {
          from += idx[k] * strides_[k];
          to += idx[k] * fresh.strides_[k];
        }
        fresh.data_[to] = data_[from];
        std::size_t k = N;
        while (k != 0) {
          if (++idx[k - 1] != common[k - 1]) break;
          idx[k - 1] = 0;
          --k;
        }
        if (k == 0) break;
      }
    }
    data_.swap(fresh.data_);
    for (std::size_t k = 0; k != N; ++k) {
      shape_[k] = fresh.shape_[k];
      strides_[k] = fresh.strides_[k];
    }
  }

  reference operator[](index i) {
    return detail::multi_array::sub_of<T, N>::get(data_.data(), shape_, strides_, i);
  }
  const_reference operator[](index i) const {
    return detail::multi_array::sub_of<const T, N>::get(data_.data(), shape_, strides_, i);
  }

  size_type size() const { return shape_[0]; }
  const size_type* shape() const { return shape_; }
  const size_type* strides() const { return strides_; }
  size_type num_elements() const { return data_.size(); }
  size_type num_dimensions() const { return N; }
  T* data() { return data_.data(); }
  const T* data() const { return data_.data(); }
  T* origin() { return data_.data(); }
  const T* origin() const { return data_.data(); }

 private:
  static detail::multi_array::extent_gen<N> zero_extents() {
    detail::multi_array::extent_gen<N> e;
    for (std::size_t k = 0; k != N; ++k) e.ext[k] = 0;
    return e;
  }
  void set_shape(const detail::multi_array::extent_gen<N>& e) {
    for (std::size_t k = 0; k != N; ++k) shape_[k] = e.ext[k];
    size_type s = 1;
    for (std::size_t k = N; k != 0; --k) {
      strides_[k - 1] = s;
      s *= shape_[k - 1];
    }
  }
  size_type total() const {
    size_type n = 1;
    for (std::size_t k = 0; k != N; ++k) n *= shape_[k];
    return n;
  }

  std::vector<T> data_;
  size_type shape_[N];
  size_type strides_[N];
};

}  // namespace boost

#endif
