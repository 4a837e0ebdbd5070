// Stand-in for <boost/shared_ptr.hpp> (test infrastructure only):
// boost::shared_ptr is std::shared_ptr.
#ifndef SKREF_STANDIN_BOOST_SHARED_PTR_HPP
#define SKREF_STANDIN_BOOST_SHARED_PTR_HPP
#include <memory>
namespace boost {
using std::shared_ptr;
}
#endif
