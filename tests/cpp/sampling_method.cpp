// BPMatrix::Options with n_samples > 0 (the reference's SFOLD method,
// common/bpmatrix.cpp:84-93) is accepted by the compatibility header's fold
// step; alifold is still refused there.  Prints one line per case.
#include <iostream>
#include <list>
#include <string>

#include "stem_kernel_compat.hpp"

static void run(const char* name, const skc::BPMatrix::Options& opts) {
  std::list<std::string> ma;
  ma.push_back("GGGGAAACCCC");
  try {
    skc::MData d(ma, 0.01f, -1.0f, opts);
    std::cout << name << ": folded " << d.bpp.size() << " row" << std::endl;
  } catch (const char* msg) {
    std::cout << name << ": error: " << msg << std::endl;
  }
}

int main() {
  skc::BPMatrix::Options opts;
  opts.n_samples = 10;
  opts.sampling_seed = 7;
  run("sampling", opts);
  opts.alifold = true;
  run("alifold", opts);
  return 0;
}
