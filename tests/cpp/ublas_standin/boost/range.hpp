// Minimal stand-in for <boost/range.hpp>.  TEST INFRASTRUCTURE ONLY: the
// const iterator of a standard container and begin / end on it, which is all
// the reference's calculate_avg_var uses.
#ifndef SK_UBLAS_STANDIN_RANGE_HPP
#define SK_UBLAS_STANDIN_RANGE_HPP

namespace boost {

template <class C>
struct range_const_iterator {
  typedef typename C::const_iterator type;
};
template <class C>
typename C::const_iterator begin(const C& c) { return c.begin(); }
template <class C>
typename C::const_iterator end(const C& c) { return c.end(); }

}  // namespace boost

#endif
