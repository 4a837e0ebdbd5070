// A reference-shaped simpal tool (the shape of simpal/simpal.cpp:282-423):
// Example = (label, Pals), load_examples over the legacy Fasta reader with
// ToLower, KernelFunc(tolerance), a train Gram or a test x train matrix through
// KernelMatrix, print, and the test norms through operator()(i).  The only
// engine-specific lines are the include and the optional fold hook.
//
// argv: out tolerance normalize fold(engine|synthetic) train.fa [test.fa]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <utility>
#include <vector>

#include "simpal_compat.hpp"

typedef std::pair<std::string, Pals> Example;
typedef std::vector<Example> ExampleSet;

uint load_examples(const std::string& label, Fasta& f, ExampleSet& ex, uint seed_length, uint min_loop,
                   uint max_dist) {
  while (!f.IsEOF() && f.GetNextSeq()) {
    f.ToLower();
    Pals pal(f.Seq(), seed_length, min_loop, max_dist);
    ex.push_back(Example(label, pal));
  }
  return ex.size();
}

int main(int argc, char** argv) {
  typedef double value_type;
  if (argc < 6) return 2;
  uint seed_length = 3, min_loop = 3, max_dist = 300, n_th = 1;  // simpal.cpp:314-318
  const int tolerance = std::atoi(argv[2]);
  const bool normalize = std::atoi(argv[3]) != 0;
  if (std::strcmp(argv[4], "synthetic") == 0) skc::simpal_fold() = skc::synthetic_fold;
  try {
    ExampleSet train, test;
    for (int a = 5; a < argc && a < 7; ++a) {
      std::ifstream in(argv[a]);
      if (!in.is_open()) {
        perror(argv[a]);
        return 1;
      }
      Fasta fasta(in);
      load_examples(a == 5 ? "+1" : "-1", fasta, a == 5 ? train : test, seed_length, min_loop, max_dist);
    }
    KernelFunc kernel(tolerance);
    KernelMatrix<value_type> matrix;
    if (test.empty()) {
      matrix.calculate(train, kernel, normalize, n_th);
    } else {
      matrix.calculate(test, train, kernel, true, normalize, n_th);
    }
    std::ofstream out(argv[1]);
    matrix.print(out);
    const size_t rows = test.empty() ? train.size() : test.size();
    std::printf("%u %u\n", (uint)rows, (uint)train.size());
    for (size_t i = 0; i != rows; ++i) {
      for (size_t j = 0; j != train.size(); ++j) std::printf("%.17g ", matrix((uint)i, (uint)j));
      std::printf("\n");
    }
    if (!test.empty())
      for (size_t i = 0; i != test.size(); ++i) std::printf("norm %.17g\n", matrix((uint)i));
    if (train.size() > 1) std::printf("pair %.17g\n", kernel(train[0].second, train[1].second));
  } catch (const char* e) {
    std::fprintf(stderr, "error: %s\n", e);
    return 1;
  }
  return 0;
}
