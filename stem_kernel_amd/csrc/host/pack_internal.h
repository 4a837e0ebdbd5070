// What the packer's files share (pack.cpp, pack_x.cpp, pack_y.cpp,
// pack_sweep.cpp): the per-example passes of pack_dataset and the LDS bank
// model of the IY sweep.  Everything else in those files is file-local.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "host/runtime_types.h"

namespace sk {

// ---- pack_sweep.cpp: the LDS bank model of the IY sweep and what uses it
// The IY sweep schedule of one y as pack_y's list scheduling leaves it:
// edges (child, parent in ids sorted by length, record er), the chunks'
// edges in schedule order, and each node's edges as a child.
struct SweepSchedule {
  int nl = 0;
  std::vector<uint32_t> er;
  std::vector<int> epar, ech;
  std::vector<int> cb, by_child;        // CSR: a child's edges
  std::vector<int> chunk_off, chunk_ed;  // CSR: a chunk's edges
  bool lanes_greedy = true;
  int nch() const { return (int)chunk_off.size() - 1; }
};
struct SweepCost {
  long read = 0, atomic = 0;
  long sum() const { return read + atomic; }
};
// the bank model's cycles of one chunk's 64 lane records
void sweep_chunk_cost(const uint32_t lanes[64], int* read_cycles, int* atomic_cycles);
// one chunk's 64 lane records: dealt to the 16-lane groups through the bank
// model (greedy) or in schedule order, padded with dummy records
void sweep_chunk_lanes(const int* take, int n, const std::vector<uint32_t>& er, int nl, bool greedy,
                       uint32_t lanes[64]);
void renumber_equal_lengths(const SweepSchedule& S, const std::vector<int>& len, std::vector<int>& newid,
                            SweepCost& plain, SweepCost& now);
void match_gather_cost(const std::vector<uint32_t>& child, const std::vector<int>& starts, long* cycles,
                       long* groups);

// ---- pack_y.cpp
// y-role records of one example (its nodes sorted by length, the IY sweep
// schedule, node-major edges), formed from its x-role arrays once pack_dataset
// has packed them: independent per example, so they run on host threads and
// are appended in example order (bit-identical to a serial pass)
struct YJob {
  int nb0, ebase, bbase, nl;
  bool big;
};
// (the records that depend on the order of the nodes, and src: y id -> the
// example's level-order node)
struct YRec {
  std::vector<uint32_t> ysc, ye2, yn_a, yn_b, yn_c, src;
  std::vector<uint4> yrec;
  std::vector<float> yn_w, yn_nbp, yn_p0;
  std::vector<double> yn_P;
};
// the records in the plain stable order by length (HostPack's yn_* / ye2 /
// ysc, as ever) and, where YOpts::renumber, in r the same records with the
// equal-length nodes renumbered (HostPack's r_*: what the device gets)
struct YOut : YRec {
  YRec r;
  std::vector<int32_t> ycs;
  int nch = 0;
  // the sweep chunks' bank-model cost in the plain order by length and as
  // packed, and whether the renumbering pass changed the order
  SweepCost cost_plain, cost;
  bool renumbered = false;
  long mg_plain = 0, mg_now = 0, mg_groups = 0;  // match_gather_cost of both orders (YOpts::stats)
  std::string err;
};
struct YOpts {
  bool sweep_lanes_greedy = true;  // SK_SWEEP_LANES=0: sweep chunks in schedule order (A/B diagnostics)
  bool renumber = true;  // renumber_equal_lengths (SK_NO_Y_RENUMBER=1: the plain stable order)
  bool stats = false;    // SK_PACK_STATS: the MATCH gather's read model too
};
YOpts y_opts_from_env();
void pack_y(const HostPack& P, const YOpts& opt, const YJob& J, YOut& Y);

// ---- pack_x.cpp
// The dataset's key tables: the (code, len) keys of its gamma rows and the
// (child key, code, len) keys of its phi rows' components, each one sorted
// set, and whether the gamma schedule uses them.
struct KeyTables {
  std::vector<uint32_t> gam_key;  // (empty unless gam_on)
  std::vector<uint64_t> phi_raw;  // child gamma key:32 | code:16 | len:16 (sorted: by child key)
  bool gam_on = false, phi_on = false;
  // the factored gamma schedule (shared child sums, pack_shared_sums.cpp)
  // and its group-value threshold
  bool ss_on = false;
  int ss_thr = 0;
  uint32_t gamma_idx(uint32_t key) const {
    return (uint32_t)(std::lower_bound(gam_key.begin(), gam_key.end(), key) - gam_key.begin());
  }
  uint32_t phi_idx(uint32_t key_p, uint32_t key_c) const {
    const uint64_t k = ((uint64_t)key_c << 32) | key_p;
    return (uint32_t)(std::lower_bound(phi_raw.begin(), phi_raw.end(), k) - phi_raw.begin());
  }
};
KeyTables key_tables(const std::vector<Example>& ex, int nthr);
// x-role records of one example (nodes in level order, the x schedules,
// per-position tables), formed per example on host threads and appended
// in example order by pack_dataset (bit-identical to one serial pass;
// example-local offsets, the dataset's bases added when appending)
struct XOut {
  std::vector<uint32_t> nd_a, nd_b, nd_c, xr_ch, xr_node, gr_info, xg_ch, xg_clg, phk_idx, gra_gidx,
      gra_row, xg_node;
  std::vector<float> nd_w, nd_nbp, bpf_p, gr_pf, xg_cpf, ex_nseqs, pos_w;
  std::vector<double> nd_P, gr_P;
  std::vector<uint2> ed;
  std::vector<uint32_t> bpf_code;
  std::vector<int32_t> lvl, ex_nslots, ex_nlxg, ex_gapless, ex_nl, ex_nlev, ex_len, ex_has_w;
  std::vector<uint8_t> ex_big, xg_cty, pos_chr, ex_dyadic, ex_str_fast, ex_onehot;
  std::vector<sk::XRow> xrow, xgrow;
  std::vector<float4> pos_prof, pos_lru;
  std::vector<uint64_t> ex_phi_bits;
  // the factored gamma schedule (empty unless K.ss_on)
  std::vector<sk::XRow> xf_row;
  std::vector<uint32_t> xf_node, xf_ch, xf_clg, xf_gra_row;
  std::vector<float> xf_cpf;
  std::vector<uint8_t> xf_cty;
  int ss_rows = 0, ss_repl = 0;
  int nl = 0, nlev = 0, max_slots = 0, n_nostore = 0, n_nodes = 0, gslots = 0;
  bool big = false;
  int rc = SK_OK;
  std::string err;
};
void pack_x(const Example& X, const KeyTables& K, XOut& O);

// ---- pack.cpp
// every position's bpla_weight, appended to out (the x role's pos_lru)
void bpla_weights(const Example& X, std::vector<float4>& out);

}  // namespace sk
