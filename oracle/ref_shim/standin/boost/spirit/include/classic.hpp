// Stand-in for <boost/spirit/include/classic.hpp> (test infrastructure only):
// the reference's file loaders hold a file_iterator<> member; the DP shims
// never open a file, so an iterator that is always "not open" is enough.
#ifndef SKREF_STANDIN_BOOST_SPIRIT_CLASSIC_HPP
#define SKREF_STANDIN_BOOST_SPIRIT_CLASSIC_HPP
#include <string>
#define BOOST_SPIRIT_CLASSIC_NS boost::spirit::classic
namespace boost { namespace spirit { namespace classic {
template <class CharT = char>
class file_iterator {
 public:
  file_iterator() {}
  explicit file_iterator(const std::string&) {}
  operator bool() const { return false; }
};
}}}
#endif
