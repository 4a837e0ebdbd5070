// BPMatrix::Options::consensus (the engine's own option) is accepted by the
// compatibility header's fold step and leaves ONE matrix over the alignment's
// columns; n_samples > 0 wins over it; alifold is still refused.  Prints one
// line per case.
#include <iostream>
#include <list>
#include <string>

#include "stem_kernel_compat.hpp"

static void run(const char* name, const skc::BPMatrix::Options& opts) {
  std::list<std::string> ma;
  ma.push_back("GGGGA-AACCCC");
  ma.push_back("GGCGAAAACGCC");
  try {
    skc::MData d(ma, 0.01f, -1.0f, opts);
    std::cout << name << ": " << d.bpp.size() << " matrices, first of " << d.bpp.front().size()
              << ", consensus " << d.consensus << std::endl;
  } catch (const char* msg) {
    std::cout << name << ": error: " << msg << std::endl;
  }
}

int main() {
  skc::BPMatrix::Options opts;
  opts.consensus = true;
  run("consensus", opts);
  opts.n_samples = 10;
  run("sampling", opts);
  opts.n_samples = 0;
  opts.alifold = true;
  run("alifold", opts);
  return 0;
}
