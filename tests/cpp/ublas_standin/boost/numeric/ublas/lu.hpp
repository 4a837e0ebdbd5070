// Stand-in for <boost/numeric/ublas/lu.hpp>: the reference includes it and uses
// nothing from it in the code that is compiled.  TEST INFRASTRUCTURE ONLY.
