// Stand-in for <boost/program_options.hpp> (test infrastructure only): just
// the names the reference's simpal main uses, so that it compiles.  Nothing
// here parses a command line; the harness never calls that main.
#ifndef SK_SIMPAL_STANDIN_BOOST_PROGRAM_OPTIONS_HPP
#define SK_SIMPAL_STANDIN_BOOST_PROGRAM_OPTIONS_HPP
#include <cstdio>
#include <ostream>
#include <string>
#include <vector>
namespace boost {
namespace program_options {
template <class T>
struct typed_value {
  typed_value* default_value(const T&) { return this; }
};
template <class T>
typed_value<T>* value(T*) {
  static typed_value<T> v;
  return &v;
}
struct options_description_easy_init {
  options_description_easy_init& operator()(const char*, const char*) { return *this; }
  template <class T>
  options_description_easy_init& operator()(const char*, typed_value<T>*, const char*) {
    return *this;
  }
};
struct options_description {
  explicit options_description(const char*) {}
  options_description_easy_init add_options() { return options_description_easy_init(); }
};
inline std::ostream& operator<<(std::ostream& os, const options_description&) { return os; }
struct option {
  bool unregistered;
};
struct parsed_options {
  std::vector<option> options;
};
enum collect_unrecognized_mode { include_positional, exclude_positional };
inline std::vector<std::string> collect_unrecognized(const std::vector<option>&, collect_unrecognized_mode) {
  return std::vector<std::string>();
}
struct command_line_parser {
  command_line_parser(int, char**) {}
  command_line_parser& options(const options_description&) { return *this; }
  command_line_parser& allow_unregistered() { return *this; }
  parsed_options run() { return parsed_options(); }
};
struct variables_map {
  unsigned count(const char*) const { return 0; }
};
inline void store(const parsed_options&, variables_map&) {}
inline void notify(variables_map&) {}
}  // namespace program_options
}  // namespace boost
#endif
