// Harness for oracle/_ref/libskref_str.so: the reference's own, unmodified
// string_kernel/string_kernel.cpp (the naive gapped string kernel on raw
// strings), compiled in place by oracle/Makefile, behind a C ABI.
#include <string>
#include "string_kernel.h"

extern "C" double sks_kernel(const char* x, const char* y, double gap) {
  return StringKernel<double>(gap)(std::string(x), std::string(y));
}
