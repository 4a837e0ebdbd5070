// Stand-in for <boost/bind.hpp> (test infrastructure only): bind(&T::member,
// _1), the one form the reference's simpal main uses.
#ifndef SK_SIMPAL_STANDIN_BOOST_BIND_HPP
#define SK_SIMPAL_STANDIN_BOOST_BIND_HPP
namespace boost {
template <int N>
struct arg {};
template <class M, class T>
struct member_reader {
  M T::*p;
  const M& operator()(const T& o) const { return o.*p; }
};
template <class M, class T>
member_reader<M, T> bind(M T::*p, arg<1>) {
  member_reader<M, T> r = {p};
  return r;
}
}  // namespace boost
static boost::arg<1> _1;
#endif
