// Host pieces of the GPU folds (the batch driver, which needs the context,
// is in host/fold_gpu.cpp): the Boltzmann tables, the nucleotide codes, the
// --noLonelyPairs pair filters and the batch plan.  No GPU call in here.
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

#include "kernels/launch.h"

namespace sk {

// Boltzmann factor tables of fold.hip (host/fold_params.h) in one buffer t,
// their offsets and lengths into L; max_len: the batch's longest item
void fold_tables(int max_len, FoldLaunch& L, std::vector<double>& t);
// the consensus fold's row energies, appended to fold_tables' (L.o_ali): 8 x 8
// stack energies by energy type, then kT, TerminalAU, bulge(1)
void fold_tables_ali(FoldLaunch& L, std::vector<double>& t);

// the codes of n characters: A C G U (T) = 0..3 in either case, anything else -1
void fold_codes(const char* s, size_t n, int8_t* out);

// --noLonelyPairs: lp[i*n + j] = 1 where the pair survives (c: n codes)
void lonely_pair_table(const int8_t* c, int n, bool no_gu, uint8_t* lp);
// the same walk over the column pairs the consensus fold's covariance score
// allows (c: n_rows rows of n codes)
void lonely_pair_table_ali(const int8_t* c, int n_rows, int n, bool no_gu, uint8_t* lp);

// The end of the batch that starts at item b0 of n: the items whose bytes
// (bytes(k)) fit the budget together, at least one
int32_t fold_batch_end(int32_t b0, int32_t n, double budget, const std::function<double(int32_t)>& bytes);

}  // namespace sk
