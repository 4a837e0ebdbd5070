// Stand-in for <boost/program_options.hpp> (test infrastructure only): the
// reference's DP headers only name options_description in a declaration.
#ifndef SKREF_STANDIN_BOOST_PROGRAM_OPTIONS_HPP
#define SKREF_STANDIN_BOOST_PROGRAM_OPTIONS_HPP
#include "shared_ptr.hpp"
namespace boost { namespace program_options {
class options_description;
}}
#endif
