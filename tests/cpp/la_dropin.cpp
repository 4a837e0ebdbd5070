// A reference-shaped la_kernel tool (the shape of bpla_kernel/la_main.cpp:118-135
// and App<K,LDF>::train, common/framework.h:121-165): the 23x23 score table,
// `LDF ldf;` for DataLoaderFactory<DataLoader<AAMData> >,
// BPLAKernel<double,AAMData> with noBP = true, examples read through the
// factory's loader and a train Gram through KernelMatrix.  The only
// engine-specific line is the include.
//
// argv: out SW normalize train(.fa|.aln|.maf)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <utility>
#include <vector>

#include "bpla_kernel_compat.hpp"

const uint N_AA = AAProfileSequence::N_AA;

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const bool SW = std::atoi(argv[2]) != 0, normalize = std::atoi(argv[3]) != 0;
  const float gap = -10.0f, ext = -1.0f, alpha = 1.0f, beta = 0.11f;  // la_main.cpp:73-76, 87-90
  // the default table of the engine (BLOSUM62), as la_main.cpp:122-126 copies its own
  sk_kernel_params def;
  sk_kernel_params_default(&def, SK_AA_LA);
  std::vector<std::vector<double> > score_table(N_AA, std::vector<double>(N_AA));
  for (uint i = 0; i != N_AA; ++i)
    for (uint j = 0; j != N_AA; ++j) score_table[i][j] = def.aa_score_table[i * N_AA + j];
  try {
    typedef DataLoaderFactory<DataLoader<AAMData> > LDF;
    LDF ldf;
    BPLAKernel<double, AAMData> kernel(score_table, true, SW, gap, ext, alpha, beta);
    std::vector<std::pair<std::string, AAMData> > ex;
    LDF::Loader* loader = ldf.get_loader(argv[4]);
    while (AAMData* d = loader->get()) {
      ex.push_back(std::make_pair(std::string(ex.size() % 2 ? "-1" : "+1"), *d));
      delete d;
    }
    delete loader;
    for (size_t i = 0; i != ex.size(); ++i)
      std::printf("example %u: %u columns, %g rows, char2aa('w') = %d\n", (uint)i, ex[i].second.size(),
                  ex[i].second.seq.n_seqs(), AAProfileSequence::char2aa('w'));
    KernelMatrix<double> matrix;
    matrix.calculate(ex, kernel, normalize, 1);
    std::ofstream out(argv[1]);
    matrix.print(out);
    for (size_t i = 0; i != ex.size(); ++i) {
      for (size_t j = 0; j != ex.size(); ++j) std::printf("%.17g ", matrix((uint)i, (uint)j));
      std::printf("\n");
    }
    if (ex.size() > 1) std::printf("pair %.17g\n", kernel(ex[0].second, ex[1].second));
  } catch (const char* e) {
    std::fprintf(stderr, "error: %s\n", e);
    return 1;
  }
  return 0;
}
