// Stand-in for <boost/algorithm/string.hpp> (test infrastructure only): the
// reference's simpal.cpp includes it and uses nothing of it.
