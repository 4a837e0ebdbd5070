// Stand-in for <boost/version.hpp> (test infrastructure only): a version new
// enough that the reference picks the "classic" Spirit include path.
#ifndef SKREF_STANDIN_BOOST_VERSION_HPP
#define SKREF_STANDIN_BOOST_VERSION_HPP
#define BOOST_VERSION 105300
#endif
