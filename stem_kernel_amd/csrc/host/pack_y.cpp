// The y role of one example (pack_y, host/pack_internal.h), in phases: its
// nodes ordered by length, the IY sweep's list schedule, the chunks' lane
// records, and the node-major records -- the last two once in the plain
// order and once in the order renumber_equal_lengths chooses.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <numeric>
#include <queue>
#include <vector>

#include "host/pack_internal.h"

namespace sk {
namespace {

// y-role numbering for the stem kernel: nodes sorted by length (span
// last - first), so the nodes inside a row's length band are one index
// range and a node's children (strictly shorter) come before it.  The order
// inside a run of equal lengths is free: srt is the stable one.
struct YOrder {
  std::vector<int> srt;  // y id -> the example's level-order node
  std::vector<int> pos;  // its inverse
};
YOrder order_by_length(const HostPack& P, const YJob& J) {
  YOrder o;
  o.srt.resize(J.nl);
  std::iota(o.srt.begin(), o.srt.end(), 0);
  auto len_of = [&](int k) { return P.nd_b[J.nb0 + k] & 0xffff; };
  std::stable_sort(o.srt.begin(), o.srt.end(), [&](int a, int b) { return len_of(a) < len_of(b); });
  o.pos.resize(J.nl);
  for (int i = 0; i < J.nl; ++i) o.pos[o.srt[i]] = i;
  return o;
}

// IY sweep schedule.  Edges are grouped by parent level (the IY sweep walks
// levels) and contiguous per parent, packed child:11 | parent:11 | gaps:10 in
// sorted ids.  The sweep is a stream of chunks of 64 edges: a chunk's
// R[child] reads are issued after the previous chunk's atomics, so an edge
// may go into any chunk after the one holding the last edge of its child
// (every node's value is final by then).  List scheduling, priority = height
// of the parent (longest path up to a root; the critical chain first), then
// the child's length; chunks are padded with dummy records (child == parent:
// weight 0) when their lanes are emitted.  cm: per chunk, the prefix maximum
// of the children's lengths.  False: the DAG has a cycle.
bool schedule_sweep(const HostPack& P, const YJob& J, const YOrder& o, SweepSchedule& S, std::vector<int32_t>& cm) {
  const int nl = J.nl, nb0 = J.nb0;
  const std::vector<int>&srt = o.srt, &pos = o.pos;
  S.nl = nl;
  std::vector<uint32_t>& er = S.er;  // records child:11 | parent:11 | gaps:10
  std::vector<int>&epar = S.epar, &ech = S.ech;
  for (int k = 0; k < nl; ++k) {
    const uint32_t a = P.nd_a[nb0 + k];
    const uint32_t ne = (a >> 16) & 0xff, el = a & 0xffff;
    for (uint32_t t = 0; t < ne; ++t) {
      const uint2 rec = P.ed[J.ebase + el + t];  // {child | gaps<<16, parent}
      const int c = pos[rec.x & 0xffff], q = pos[k];
      epar.push_back(q);
      ech.push_back(c);
      er.push_back((uint32_t)c | ((uint32_t)q << 11) | ((rec.x >> 16) << 22));
    }
  }
  const int ne_all = (int)er.size();
  // a child's edges in edge order (CSR: one allocation, not one per node)
  std::vector<int>&cb = S.cb, &by_child = S.by_child;
  cb.assign(nl + 1, 0);
  by_child.resize(ne_all);
  for (int f = 0; f < ne_all; ++f) cb[ech[f] + 1]++;
  for (int i = 0; i < nl; ++i) cb[i + 1] += cb[i];
  {
    std::vector<int> fillc(cb.begin(), cb.end() - 1);
    for (int f = 0; f < ne_all; ++f) by_child[fillc[ech[f]]++] = f;
  }
  // sorted ids: a parent is strictly longer, so it has a larger id
  std::vector<int> h(nl, 0), rem(nl, 0);
  for (int i = nl - 1; i >= 0; --i)
    for (int t = cb[i]; t < cb[i + 1]; ++t) h[i] = std::max(h[i], h[epar[by_child[t]]] + 1);
  for (int f = 0; f < ne_all; ++f) rem[epar[f]]++;
  // key (-height, child len, edge) packed into one integer, smallest
  // first: 2^20 - 1 - height:20 | len:16 | edge:28 (nl < 2^16, edges < 2^28)
  std::priority_queue<uint64_t, std::vector<uint64_t>, std::greater<uint64_t>> ready;
  auto push_edges_of = [&](int c) {
    const uint64_t len = P.nd_b[nb0 + srt[c]] & 0xffff;
    for (int t = cb[c]; t < cb[c + 1]; ++t) {
      const int f = by_child[t];
      ready.push(((uint64_t)((1 << 20) - 1 - h[epar[f]]) << 44) | (len << 28) | (uint64_t)f);
    }
  };
  for (int c = 0; c < nl; ++c)
    if (rem[c] == 0) push_edges_of(c);
  int32_t run = -1, placed = 0;
  // done: parents completed by the chunk just formed; their edges are
  // ready from the next chunk on
  std::vector<int> take, done;
  S.chunk_off.push_back(0);
  while (!ready.empty()) {
    take.clear();
    done.clear();
    while (!ready.empty() && (int)take.size() < 64) {
      take.push_back((int)(ready.top() & 0xfffffffu));
      ready.pop();
    }
    for (int f : take) {
      run = std::max<int32_t>(run, (int32_t)(P.nd_b[nb0 + srt[ech[f]]] & 0xffff));
      if (--rem[epar[f]] == 0) done.push_back(epar[f]);
    }
    S.chunk_ed.insert(S.chunk_ed.end(), take.begin(), take.end());
    S.chunk_off.push_back((int)S.chunk_ed.size());
    placed += (int)take.size();
    cm.push_back(run);
    for (int q : done) push_edges_of(q);  // ready from the next chunk on
  }
  return placed == ne_all;
}

// the chunks' records (recs: S.er in some numbering) dealt to the lanes,
// appended to A.ysc; their bank-model cost
SweepCost emit_lanes(const SweepSchedule& S, const std::vector<uint32_t>& recs, YRec& A) {
  SweepCost dealt;
  for (int c = 0; c < S.nch(); ++c) {
    uint32_t lanes[64];
    int rd, at;
    sweep_chunk_lanes(S.chunk_ed.data() + S.chunk_off[c], S.chunk_off[c + 1] - S.chunk_off[c], recs, S.nl,
                      S.lanes_greedy, lanes);
    sweep_chunk_cost(lanes, &rd, &at);
    dealt.read += rd;
    dealt.atomic += at;
    A.ysc.insert(A.ysc.end(), lanes, lanes + 64);
  }
  return dealt;
}

// node records in the order o, with the node-major copy of the edges (the
// MATCH sums of a run of consecutive nodes read one contiguous edge range); a
// node's record keeps its first edge there, E(q) = prefix sum of n_edges
void emit_nodes(const HostPack& P, const YJob& J, const YOrder& o, YRec& Y) {
  const int nb0 = J.nb0;
  const int ye2_base = (int)Y.ye2.size();
  for (int i = 0; i < J.nl; ++i) {
    const int k = o.srt[i];
    Y.src.push_back((uint32_t)k);
    const uint32_t a = P.nd_a[nb0 + k];
    const uint32_t ne = (a >> 16) & 0xff, el = a & 0xffff;
    const uint32_t nbf = a >> 24, bl = P.nd_b[nb0 + k] >> 16;
    Y.yn_a.push_back(((uint32_t)Y.ye2.size() - ye2_base) | (a & 0xffff0000u));
    for (uint32_t t = 0; t < ne; ++t) {
      const uint2 rec = P.ed[J.ebase + el + t];
      Y.ye2.push_back(J.big ? 0u : (uint32_t)o.pos[rec.x & 0xffff] | ((uint32_t)i << 11) | ((rec.x >> 16) << 22));
    }
    // c = loop leaf-edge gaps:16 | first bp-freq code:4 | single-entry flag
    // (one bp-freq entry, no gap column: the closed-form node score)
    const bool one = nbf == 1 && P.nd_nbp[nb0 + k] == 0.0f;
    const uint32_t bc0 = nbf ? P.bpf_code[J.bbase + bl] & 0xf : 0u;
    Y.yn_c.push_back((P.nd_c[nb0 + k] & 0xffff) | (bc0 << 16) | ((one ? 1u : 0u) << 24));
    Y.yn_p0.push_back(nbf ? P.bpf_p[J.bbase + bl] : 0.0f);
    {
      uint4 r;
      r.x = Y.yn_a.back();
      r.y = Y.yn_c.back();
      std::memcpy(&r.z, &P.nd_w[nb0 + k], 4);
      std::memcpy(&r.w, &Y.yn_p0.back(), 4);
      Y.yrec.push_back(r);
    }
    Y.yn_b.push_back(P.nd_b[nb0 + k]);
    Y.yn_w.push_back(P.nd_w[nb0 + k]);
    Y.yn_nbp.push_back(P.nd_nbp[nb0 + k]);
    Y.yn_P.push_back(P.nd_P[nb0 + k]);
  }
}

// the MATCH gather's reads in both orders, from every length's first edge (YOpts::stats)
void gather_stats(YOut& Y) {
  std::vector<int> starts;
  std::vector<uint32_t> now, plain;
  for (size_t i = 0; i < Y.yn_b.size(); ++i)
    if (i == 0 || (Y.yn_b[i] & 0xffff) != (Y.yn_b[i - 1] & 0xffff)) starts.push_back((int)(Y.yn_a[i] & 0xffff));
  for (uint32_t e : Y.r.ye2) now.push_back(e & 0x7ff);
  for (uint32_t e : Y.ye2) plain.push_back(e & 0x7ff);
  long g2 = 0;
  match_gather_cost(now, starts, &Y.mg_now, &Y.mg_groups);
  match_gather_cost(plain, starts, &Y.mg_plain, &g2);
}

}  // namespace

YOpts y_opts_from_env() {
  YOpts opt;
  const char* lanes_env = SK_KNOB("SK_SWEEP_LANES");
  opt.sweep_lanes_greedy = !lanes_env || std::atoi(lanes_env) != 0;
  opt.renumber = !SK_KNOB("SK_NO_Y_RENUMBER");
  opt.stats = std::getenv("SK_PACK_STATS") != nullptr;
  return opt;
}

void pack_y(const HostPack& P, const YOpts& opt, const YJob& J, YOut& Y) {
  const int nl = J.nl;
  const YOrder plain = order_by_length(P, J);
  YOrder renum;  // the renumbered order (Y.r), where the pass changed the plain one
  auto len_of = [&](int i) { return (int)(P.nd_b[J.nb0 + plain.srt[i]] & 0xffff); };
  const int lmax = nl ? len_of(nl - 1) : 0;
  if (J.big) {  // no sweep schedule: the big-y kernel walks the levels (and Y.r keeps the plain order)
    Y.ycs.insert(Y.ycs.end(), lmax + 2, 0);
    Y.nch = 0;
  } else {
    SweepSchedule S;
    S.lanes_greedy = opt.sweep_lanes_greedy;
    std::vector<int32_t> cm;
    if (!schedule_sweep(P, J, plain, S, cm)) {
      Y.err = "IY sweep schedule: DAG has a cycle";
      return;
    }
    // the chunks are composed: their records dealt to the lanes in the
    // plain order, then in the order renumber_equal_lengths chooses inside
    // the runs of equal length
    Y.cost_plain = Y.cost = emit_lanes(S, S.er, Y);
    if (opt.renumber) {
      std::vector<int> len(nl), newid;
      for (int i = 0; i < nl; ++i) len[i] = len_of(i);
      renumber_equal_lengths(S, len, newid, Y.cost_plain, Y.cost);
      for (int i = 0; i < nl && !Y.renumbered; ++i) Y.renumbered = newid[i] != i;
      if (Y.renumbered) {
        renum.srt.resize(nl);
        renum.pos.resize(nl);
        for (int i = 0; i < nl; ++i) renum.srt[newid[i]] = plain.srt[i];
        for (int i = 0; i < nl; ++i) renum.pos[renum.srt[i]] = i;
        for (uint32_t& r : S.er)
          r = (r & ~0x3fffffu) | (uint32_t)newid[r & 0x7ff] | ((uint32_t)newid[(r >> 11) & 0x7ff] << 11);
        emit_lanes(S, S.er, Y.r);
      } else {
        Y.r.ysc = Y.ysc;
      }
    }
    // first chunk whose prefix maximum reaches v, v = 0 .. lmax+1
    Y.nch = S.nch();
    for (int v = 0, c = 0; v <= lmax + 1; ++v) {
      while (c < Y.nch && cm[c] < v) ++c;
      Y.ycs.push_back(c);
    }
  }
  emit_nodes(P, J, plain, Y);
  if (opt.renumber) emit_nodes(P, J, Y.renumbered ? renum : plain, Y.r);
  if (opt.stats && opt.renumber && !J.big) gather_stats(Y);
}

}  // namespace sk
