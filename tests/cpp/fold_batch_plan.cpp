// The host pieces of the GPU folds (csrc/host/fold_host.h) on their own, no
// GPU code: the batch plan of a fold call and the --noLonelyPairs tables.
//
//   fold_batch_plan plan BUDGET LEN...  one line per batch the plain fold makes
//                                       of sequences of these lengths under a
//                                       budget of BUDGET bytes: "LEN:BYTES ..."
//   fold_batch_plan lonely SEQ          the lonely-pair table of SEQ must equal
//                                       the consensus fold's table of SEQ given
//                                       as one row and as three equal rows,
//                                       with and without --noGU; prints the
//                                       number of surviving pairs of each
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host/fold_host.h"

static int plan(int argc, char** argv) {
  const double budget = std::atof(argv[2]);
  std::vector<size_t> len;
  for (int k = 3; k < argc; ++k) len.push_back((size_t)std::atol(argv[k]));
  const int32_t n = (int32_t)len.size();
  auto bytes = [&](int32_t k) { return (double)sk::fold_work_doubles(len[k]) * 8.0; };
  for (int32_t b0 = 0; b0 < n;) {
    const int32_t b1 = sk::fold_batch_end(b0, n, budget, bytes);
    if (b1 <= b0) return 1;  // a batch holds at least one item
    for (int32_t k = b0; k < b1; ++k) std::printf("%s%zu:%.0f", k > b0 ? " " : "", len[k], bytes(k));
    std::printf("\n");
    b0 = b1;
  }
  return 0;
}

static int lonely(const char* seq) {
  const int n = (int)std::strlen(seq);
  std::vector<int8_t> c(3 * (size_t)n);
  for (int r = 0; r < 3; ++r) sk::fold_codes(seq, (size_t)n, c.data() + (size_t)r * n);
  for (int no_gu = 0; no_gu < 2; ++no_gu) {
    std::vector<uint8_t> one((size_t)n * n, 7), ali1(one), ali3(one);
    sk::lonely_pair_table(c.data(), n, no_gu != 0, one.data());
    sk::lonely_pair_table_ali(c.data(), 1, n, no_gu != 0, ali1.data());
    sk::lonely_pair_table_ali(c.data(), 3, n, no_gu != 0, ali3.data());
    if (one != ali1 || one != ali3) {
      std::printf("no_gu %d: tables differ\n", no_gu);
      return 1;
    }
    int pairs = 0;
    for (uint8_t v : one) pairs += v;
    std::printf("no_gu %d: %d pairs\n", no_gu, pairs);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !std::strcmp(argv[1], "plan")) return plan(argc, argv);
  if (argc == 3 && !std::strcmp(argv[1], "lonely")) return lonely(argv[2]);
  std::fprintf(stderr, "usage: fold_batch_plan plan BUDGET LEN... | lonely SEQ\n");
  return 2;
}
