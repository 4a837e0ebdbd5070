// The factored gamma schedule of one example (pack_shared_sums.cpp): the
// gamma schedule's rows plus shared-sum combination rows, which hold the
// weighted sum of a set of children that several swept rows read, so that
// each of those rows reads one row in place of the set.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "kernels/device_set.h"

namespace sk {

// one child record of a gamma-schedule row
struct SsRec {
  int32_t row;   // the child's row (index into the schedule's rows), -1: a table row (gamma child, phi component)
  uint32_t key;  // table rows: the child's identity (its DAG node for a gamma child)
  uint32_t lo;   // table rows: the record's low 16 bits (0x8000 | gamma index, 0x4000 | phi index)
  uint32_t gaps, clg;
  float cpf;
  uint8_t cty;
};
struct SsRow {
  XRow xr;        // the row's record (the child count in a and the slot in b are filled here)
  uint32_t node;  // xg_node
  bool user;      // a swept row that is no phi row: it may read shared sums
  bool swept;     // its reader may take it from registers (a row with children that is no phi row)
  std::vector<SsRec> rec;
};
struct SsOut {
  std::vector<XRow> row;
  std::vector<uint32_t> node, ch, clg;
  std::vector<float> cpf;
  std::vector<uint8_t> cty;
  std::vector<uint32_t> new_index;  // input row -> its row in the factored schedule
  int nslots = 0, n_shared = 0, n_replaced = 0;
};

// The factored schedule of the rows `in` (schedule order; consumed).  A set of s
// children shared by k users becomes a row when k s - (s + 1 + k) exceeds
// `threshold`; store_all: no never-stored rows (the plain schedule's
// SK_STORE_ALL).  Returns false where the result would break a limit of the
// packed layout (the caller keeps the plain schedule for the example).
bool shared_sums_schedule(std::vector<SsRow>&& in, int threshold, bool store_all, SsOut& out);

}  // namespace sk
