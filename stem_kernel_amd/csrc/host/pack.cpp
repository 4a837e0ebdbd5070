// The packer: the host image of a dataset in the layout the kernels read
// (kernels/device_set.h) -- an RNA dataset's x-role and y-role records
// (pack_dataset, in phases: key tables, pack_x per example, pack_y per
// example), a protein dataset's and a palindrome dataset's arrays -- and the
// entry points that upload it or hash it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <numeric>
#include <queue>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "host/pack_shared_sums.h"
#include "host/runtime_types.h"

namespace sk {
namespace {

// every position's bpla_weight, appended to out, in one pass over the
// triangle's rows: the same float sums in the same order (pl[i] over j > i,
// pr[i] over j < i, both by increasing j), O(L^2) with contiguous reads
void bpla_weights(const Example& X, std::vector<float4>& out) {
  const int L = X.len;
  const size_t base = out.size();
  out.resize(base + (size_t)std::max(L, 0));
  if (!X.has_bp) {
    for (int i = 0; i < L; ++i) out[base + i] = make_float4(0.f, 0.f, 1.f, 0.f);
    return;
  }
  std::vector<float> pr((size_t)L, 0.0f);
  for (int i = 0; i < L; ++i) {
    float pl = 0.0f;
    if (i + 1 < L) {
      const double* row = X.bpp.data() + sk::tri_index(L, i, i + 1);
      for (int j = i + 1; j < L; ++j) {
        const double b = row[j - i - 1];
        pl = (float)((double)pl + b);
        pr[j] = (float)((double)pr[j] + b);
      }
    }
    float pu = (float)(1.0 - (double)(pl + pr[i]));  // pr[i] is final: rows j < i came first
    if (pu < 0.0f) pu = 0.0f;
    out[base + i] = make_float4(std::sqrt(pl), std::sqrt(pr[i]), std::sqrt(pu), 0.f);
  }
}

// Packed image of a palindrome dataset (sk::SimpalSet).
static void pack_palindromes(sk_dataset* ds) {
  sk_dataset::PalPack& P = ds->spack;
  P = sk_dataset::PalPack();
  P.ex_off.push_back(0);
  for (const Example& X : ds->ex) {
    P.key.insert(P.key.end(), X.pal_key.begin(), X.pal_key.end());
    P.dist.insert(P.dist.end(), X.pal_dist.begin(), X.pal_dist.end());
    P.w.insert(P.w.end(), X.pal_w.begin(), X.pal_w.end());
    P.ex_off.push_back((int32_t)P.key.size());
  }
}

// Packed image of a protein dataset (sk::LaProtSet): per position the 24
// counts and, in examples whose every column has one non-empty slot, that
// slot (23 elsewhere; the code kernel takes only pairs of such examples).
static void pack_protein(sk_dataset* ds) {
  sk_dataset::ProtPack& P = ds->ppack;
  P = sk_dataset::ProtPack();
  size_t pos = 0;
  for (const Example& X : ds->ex) pos += (size_t)X.len;
  P.prof.reserve(pos * sk::kAaSlots);
  P.code.reserve(pos);
  for (const Example& X : ds->ex) {
    P.ex_len.push_back(X.len);
    P.ex_pos_base.push_back((int32_t)P.code.size());
    bool coded = true;
    for (int i = 0; i < X.len; ++i) {
      const float* c = X.aa_prof.data() + (size_t)i * sk::kAaSlots;
      int used = 0, slot = sk::kAaSlots - 1;
      for (int k = 0; k < sk::kAaSlots; ++k)
        if (c[k] != 0.0f) {
          ++used;
          slot = k;
        }
      coded = coded && used == 1;
      P.code.push_back((uint8_t)slot);
    }
    if (!coded) std::fill(P.code.end() - X.len, P.code.end(), (uint8_t)(sk::kAaSlots - 1));
    P.ex_coded.push_back(coded ? 1 : 0);
    P.prof.insert(P.prof.end(), X.aa_prof.begin(), X.aa_prof.end());
  }
}

// LDS bank model of one IY sweep chunk (64 records child:11 | parent:11 |
// gaps:10 in lane order).  The kernel reads R[child] (ds_read_b64: banks by
// element mod 32 within each 32-lane half, one cycle per distinct address of
// the fullest bank) and adds into R[parent] (ds_add_f64: taken as 16-lane
// groups, element mod 16, one cycle per record of the fullest bank, same
// address or not).  The lane dealing below and the renumbering pass of pack_y
// both place records through it, and sk_dataset_sweep_conflicts reports it.
struct SweepBanks {
  int at[4][16];            // group -> parent bank -> records
  uint16_t rd[2][32][32];   // half -> child bank -> its distinct children
  int rdn[2][32];
  SweepBanks() { clear(); }
  void clear() {
    std::memset(at, 0, sizeof(at));
    std::memset(rdn, 0, sizeof(rdn));
  }
  bool has_child(int h, uint32_t c) const {
    const int sl = c & 31;
    for (int t = 0; t < rdn[h][sl]; ++t)
      if (rd[h][sl][t] == c) return true;
    return false;
  }
  // distinct children on c's bank of half h once c is read there
  int child_load(int h, uint32_t c) const { return rdn[h][c & 31] + (has_child(h, c) ? 0 : 1); }
  int parent_load(int g, uint32_t q) const { return at[g][q & 15]; }
  void put(int g, uint32_t c, uint32_t q) {
    const int h = g >> 1, sl = c & 31;
    if (!has_child(h, c)) rd[h][sl][rdn[h][sl]++] = (uint16_t)c;
    at[g][q & 15]++;
  }
  int read_cycles() const {  // per 32-lane half, the fullest bank (floor 2)
    int s = 0;
    for (int h = 0; h < 2; ++h) s += *std::max_element(rdn[h], rdn[h] + 32);
    return s;
  }
  int atomic_cycles() const {  // per 16-lane group, the fullest bank (floor 4)
    int s = 0;
    for (int g = 0; g < 4; ++g) s += *std::max_element(at[g], at[g] + 16);
    return s;
  }
};
static void sweep_chunk_cost(const uint32_t lanes[64], int* read_cycles, int* atomic_cycles) {
  SweepBanks B;
  for (int l = 0; l < 64; ++l) B.put(l >> 4, lanes[l] & 0x7ff, (lanes[l] >> 11) & 0x7ff);
  *read_cycles = B.read_cycles();
  *atomic_cycles = B.atomic_cycles();
}

// Lane placement of one IY sweep chunk (records child:11 | parent:11 |
// gaps:10, sorted ids): the edges are dealt to the four 16-lane groups
// greedily to spread the child reads and the parent atomics over the banks
// of SweepBanks, the parents with most edges in the chunk first; dummies
// (child == parent, weight 0) take the emptiest slots.
static void assign_sweep_lanes(const int* take, int n, const std::vector<uint32_t>& er, int nl,
                               uint32_t lanes[64]) {
  // n <= 64: fixed arrays, no allocation per chunk
  // edges per parent in the chunk (a per-thread count table over the 11-bit
  // parent ids, cleared again after use)
  thread_local uint8_t npar[2048];
  int cntp[64];
  for (int i = 0; i < n; ++i) ++npar[(er[take[i]] >> 11) & 0x7ff];
  for (int i = 0; i < n; ++i) cntp[i] = npar[(er[take[i]] >> 11) & 0x7ff];
  for (int i = 0; i < n; ++i) npar[(er[take[i]] >> 11) & 0x7ff] = 0;
  // edges by that count, largest first, chunk order among equals (a
  // counting sort: stable)
  int ord[64];
  {
    int cstart[66] = {0};
    for (int i = 0; i < n; ++i) ++cstart[64 - cntp[i] + 1];
    for (int k = 0; k < 65; ++k) cstart[k + 1] += cstart[k];
    for (int i = 0; i < n; ++i) ord[cstart[64 - cntp[i]]++] = i;
  }
  int fill[4] = {0, 0, 0, 0};
  SweepBanks B;
  auto put = [&](int g, uint32_t r) {
    B.put(g, r & 0x7ff, (r >> 11) & 0x7ff);
    lanes[16 * g + fill[g]++] = r;
  };
  for (int oi = 0; oi < n; ++oi) {
    const int i = ord[oi];
    const uint32_t r = er[take[i]];
    const uint32_t c = r & 0x7ff, q = (r >> 11) & 0x7ff;
    int best = -1, bc = 1 << 30;
    for (int g = 0; g < 4; ++g) {
      if (fill[g] == 16) continue;
      const int cost = 4 * (B.child_load(g >> 1, c) + B.parent_load(g, q) + 1) + fill[g];
      if (cost < bc) {
        bc = cost;
        best = g;
      }
    }
    put(best, r);
  }
  const int nl1 = std::max(nl, 1);
  for (int g = 0; g < 4; ++g) {
    while (fill[g] < 16) {
      int bs = 0, bc = 1 << 30;
      for (int sl = 0; sl < 32 && sl < nl1; ++sl) {
        const int cost = B.rdn[g >> 1][sl] + B.at[g][sl & 15];
        if (cost < bc) {
          bc = cost;
          bs = sl;
        }
      }
      const uint32_t d = (uint32_t)(bs % nl1);
      put(g, d | (d << 11));
    }
  }
}
// one chunk's 64 lane records: dealt (above) or in schedule order, padded
// with dummy records
static void sweep_chunk_lanes(const int* take, int n, const std::vector<uint32_t>& er, int nl, bool greedy,
                              uint32_t lanes[64]) {
  if (greedy) return assign_sweep_lanes(take, n, er, nl, lanes);
  for (int j = 0; j < n; ++j) lanes[j] = er[take[j]];
  for (int j = n; j < 64; ++j) {
    const uint32_t d = (uint32_t)(j % std::max(nl, 1));
    lanes[j] = d | (d << 11);
  }
}

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

// Renumbering of the y nodes within runs of equal length (len[i], by sorted
// id, non-decreasing).  Nothing but a node's LDS bank depends on its place
// inside such a run (pack_y), so the ids of a run are permuted to lower the
// SweepBanks cost summed over the y's chunks, whose composition stays as it
// is: a greedy pass (nodes by incidence, most first; each takes the free id
// of its run with the fewest same-bank children and parents already placed
// in its chunks; ties keep the node's own id, then the lowest), then a
// bounded number of swaps within runs, proposed from the same counts for
// the costliest chunk and kept when the dealt chunks' cost falls.  newid is
// the identity unless the result costs less than the plain order.
static void renumber_equal_lengths(const SweepSchedule& S, const std::vector<int>& len, std::vector<int>& newid,
                                   SweepCost& plain, SweepCost& now) {
  const int nl = S.nl, nch = S.nch(), ne = (int)S.er.size();
  newid.resize(nl);
  std::iota(newid.begin(), newid.end(), 0);
  std::vector<int> cread(nch), catom(nch);
  auto deal_cost = [&](int ch, const std::vector<uint32_t>& er, int* rd, int* at) {
    uint32_t lanes[64];
    sweep_chunk_lanes(S.chunk_ed.data() + S.chunk_off[ch], S.chunk_off[ch + 1] - S.chunk_off[ch], er, nl,
                      S.lanes_greedy, lanes);
    sweep_chunk_cost(lanes, rd, at);
  };
  plain = SweepCost();
  for (int ch = 0; ch < nch; ++ch) {
    deal_cost(ch, S.er, &cread[ch], &catom[ch]);
    plain.read += cread[ch];
    plain.atomic += catom[ch];
  }
  now = plain;
  // runs of equal length: r0[i] .. r1[i] holds i
  std::vector<int> r0(nl), r1(nl);
  bool any_run = false;
  for (int i = 0; i < nl;) {
    int j = i;
    while (j < nl && len[j] == len[i]) ++j;
    for (int t = i; t < j; ++t) r0[t] = i, r1[t] = j;
    any_run |= j - i > 1;
    i = j;
  }
  if (!any_run || nch == 0) return;
  // a node's chunks: as a child (each chunk once: one address however many
  // lanes read it) and as a parent (with its records there), CSR by node
  std::vector<int> coff(nl + 1, 0), poff(nl + 1, 0), cinc, pinc, pmul, pfirst(nl, -1), pcount(nl, 0);
  {
    std::vector<uint64_t> ck, pk;  // node:32 | chunk:24 | records:8
    std::vector<int> lastc(nl, -1), lastp(nl, -1);
    std::vector<size_t> pat(nl, 0);
    for (int ch = 0; ch < nch; ++ch)
      for (int t = S.chunk_off[ch]; t < S.chunk_off[ch + 1]; ++t) {
        const int f = S.chunk_ed[t], c = S.ech[f], q = S.epar[f];
        if (lastc[c] != ch) {
          lastc[c] = ch;
          ck.push_back(((uint64_t)c << 32) | ((uint64_t)ch << 8));
        }
        if (lastp[q] != ch) {
          lastp[q] = ch;
          pat[q] = pk.size();
          pk.push_back(((uint64_t)q << 32) | ((uint64_t)ch << 8));
        }
        ++pk[pat[q]];
      }
    std::sort(ck.begin(), ck.end());
    std::sort(pk.begin(), pk.end());
    for (uint64_t k : ck) {
      ++coff[(k >> 32) + 1];
      cinc.push_back((int)((k >> 8) & 0xffffff));
    }
    for (uint64_t k : pk) {
      ++poff[(k >> 32) + 1];
      pinc.push_back((int)((k >> 8) & 0xffffff));
      pmul.push_back((int)(k & 0xff));
    }
    for (int i = 0; i < nl; ++i) coff[i + 1] += coff[i], poff[i + 1] += poff[i];
    for (int f = ne - 1; f >= 0; --f) pfirst[S.epar[f]] = f, ++pcount[S.epar[f]];  // a parent's edges are contiguous
  }
  // placed same-bank children (distinct) and parent records per chunk
  std::vector<uint16_t> rc((size_t)nch * 32, 0), ac((size_t)nch * 16, 0);
  auto score = [&](int v, int id) {
    int s = 0;
    for (int t = coff[v]; t < coff[v + 1]; ++t) s += rc[(size_t)cinc[t] * 32 + (id & 31)];
    for (int t = poff[v]; t < poff[v + 1]; ++t) s += pmul[t] * ac[(size_t)pinc[t] * 16 + (id & 15)];
    return s;
  };
  auto place = [&](int v, int id, int sign) {
    for (int t = coff[v]; t < coff[v + 1]; ++t) rc[(size_t)cinc[t] * 32 + (id & 31)] += sign;
    for (int t = poff[v]; t < poff[v + 1]; ++t) ac[(size_t)pinc[t] * 16 + (id & 15)] += sign * pmul[t];
  };
  // greedy pass: the nodes alone in their run are where they are; the rest
  // by incidence (edges as a child and as a parent), most first, then by id
  std::vector<int> who(nl, -1);  // id -> node
  {
    std::vector<int> ord;
    for (int v = 0; v < nl; ++v) {
      if (r1[v] - r0[v] == 1) {
        place(v, v, 1);
        who[v] = v;
      } else {
        ord.push_back(v);
      }
    }
    auto inc = [&](int v) { return S.cb[v + 1] - S.cb[v] + pcount[v]; };
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return inc(a) > inc(b); });
    for (int v : ord) {
      int sc[32], best = -1;
      std::fill(sc, sc + 32, -1);
      for (int j = r0[v]; j < r1[v]; ++j) {
        if (who[j] >= 0) continue;
        if (sc[j & 31] < 0) sc[j & 31] = score(v, j);
        // lower score; then the node's own id; then the lower id (j ascends)
        if (best < 0 || sc[j & 31] < sc[best & 31] || (sc[j & 31] == sc[best & 31] && j == v)) best = j;
      }
      newid[v] = best;
      who[best] = v;
      place(v, best, 1);
    }
  }
  // the dealt cost of that numbering
  std::vector<uint32_t> er(S.er);
  auto set_id = [&](int v, int id) {
    for (int t = S.cb[v]; t < S.cb[v + 1]; ++t) er[S.by_child[t]] = (er[S.by_child[t]] & ~0x7ffu) | (uint32_t)id;
    for (int f = pfirst[v]; f >= 0 && f < pfirst[v] + pcount[v]; ++f)
      er[f] = (er[f] & ~(0x7ffu << 11)) | ((uint32_t)id << 11);
  };
  for (int v = 0; v < nl; ++v)
    if (newid[v] != v) set_id(v, newid[v]);
  now = SweepCost();
  for (int ch = 0; ch < nch; ++ch) {
    deal_cost(ch, er, &cread[ch], &catom[ch]);
    now.read += cread[ch];
    now.atomic += catom[ch];
  }
  // swaps within runs, at most kSwapTries proposals
  {
    const int kSwapTries = std::min(nch, 32);
    std::vector<uint8_t> tried(nch, 0);
    std::vector<int> aff, stamp(nch, -1), asked(nl, -1);
    for (int it = 0; it < kSwapTries; ++it) {
      int ch = -1;
      for (int k = 0; k < nch; ++k)
        if (!tried[k] && cread[k] + catom[k] > 6 && (ch < 0 || cread[k] + catom[k] > cread[ch] + catom[ch])) ch = k;
      if (ch < 0) break;
      // the nodes on the chunk's fullest child and parent banks
      int mc = 0, mp = 0;
      for (int b = 0; b < 32; ++b) mc = std::max<int>(mc, rc[(size_t)ch * 32 + b]);
      for (int b = 0; b < 16; ++b) mp = std::max<int>(mp, ac[(size_t)ch * 16 + b]);
      int ba = -1, bj = -1, bd = 0;
      auto propose = [&](int a) {
        if (r1[a] - r0[a] == 1 || asked[a] == it) return;
        asked[a] = it;
        const int ia = newid[a];
        place(a, ia, -1);
        const int sa = score(a, ia);
        for (int j = r0[a]; j < r1[a]; ++j) {
          if ((j & 31) == (ia & 31)) continue;
          const int b = who[j];
          place(b, j, -1);
          const int d = score(a, j) + score(b, ia) - sa - score(b, j);
          place(b, j, 1);
          if (d < bd || (d == bd && d < 0 && (a < ba || (a == ba && j < bj)))) bd = d, ba = a, bj = j;
        }
        place(a, ia, 1);
      };
      for (int t = S.chunk_off[ch]; t < S.chunk_off[ch + 1]; ++t) {
        const int f = S.chunk_ed[t], c = S.ech[f], q = S.epar[f];
        if (mc > 1 && rc[(size_t)ch * 32 + (newid[c] & 31)] == mc) propose(c);
        if (ac[(size_t)ch * 16 + (newid[q] & 15)] == mp) propose(q);
      }
      if (ba < 0) {
        tried[ch] = 1;
        continue;
      }
      // the chunks either node is in, dealt again with the two ids exchanged
      const int a = ba, b = who[bj], ia = newid[a], ib = bj;
      aff.clear();
      for (int v : {a, b}) {
        for (int t = coff[v]; t < coff[v + 1]; ++t)
          if (stamp[cinc[t]] != it) stamp[cinc[t]] = it, aff.push_back(cinc[t]);
        for (int t = poff[v]; t < poff[v + 1]; ++t)
          if (stamp[pinc[t]] != it) stamp[pinc[t]] = it, aff.push_back(pinc[t]);
      }
      set_id(a, ib);
      set_id(b, ia);
      long before = 0, after = 0, dr = 0, da = 0;
      std::vector<int> nr(aff.size()), na(aff.size());
      for (size_t k = 0; k < aff.size(); ++k) {
        deal_cost(aff[k], er, &nr[k], &na[k]);
        before += cread[aff[k]] + catom[aff[k]];
        after += nr[k] + na[k];
        dr += nr[k] - cread[aff[k]];
        da += na[k] - catom[aff[k]];
      }
      if (after < before) {
        for (size_t k = 0; k < aff.size(); ++k) cread[aff[k]] = nr[k], catom[aff[k]] = na[k];
        place(a, ia, -1);
        place(b, ib, -1);
        place(a, ib, 1);
        place(b, ia, 1);
        newid[a] = ib, newid[b] = ia;
        who[ib] = a, who[ia] = b;
        now.read += dr;
        now.atomic += da;
      } else {
        set_id(a, ia);
        set_id(b, ib);
        tried[ch] = 1;
      }
    }
  }
  if (now.sum() >= plain.sum()) {  // nothing gained: today's numbering
    std::iota(newid.begin(), newid.end(), 0);
    now = plain;
  }
}

// The MATCH sums gather R[child] over the node-major edges in rounds of 64
// from the first edge of a row's length band, so they read children by id
// too; their rounds' alignment depends on the band and cannot be optimised
// exactly.  The read model (SweepBanks: distinct children per bank of each
// 32-lane half) over the 64-edge groups from every start in `starts` to the
// end of the edges: cycles and groups (SK_PACK_STATS).
static void match_gather_cost(const std::vector<uint32_t>& child, const std::vector<int>& starts, long* cycles,
                              long* groups) {
  const int ne = (int)child.size();
  for (int s0 : starts)
    for (int f = s0; f < ne; f += 64) {
      SweepBanks B;
      for (int l = 0; l < 64 && f + l < ne; ++l) B.put(l >> 4, child[f + l], 0u);
      *cycles += B.read_cycles();
      ++*groups;
    }
}

// ---- the phases of pack_dataset
// Gamma rows: x loop rows (one leaf child) with one bp-frequency entry and
// no gap column.  Their G0 row is (g^gaps pf) x Gamma_{code,len}(y), the
// IY sweep of a y-only vector (dag_stem.hip), so the gamma schedule skips
// them; the dataset's (code, len) keys index the per-y Gamma rows.
bool is_gamma(const Example& X, int v) {
  const uint32_t e0 = X.edge_off[v], e1 = X.edge_off[v + 1];
  if (e1 - e0 != 1) return false;
  const uint32_t c = X.edge_to[e0];
  if (X.edge_off[c + 1] != X.edge_off[c]) return false;  // the child is not a leaf: a stem
  return X.bpf_off[v + 1] - X.bpf_off[v] == 1 && X.prof5[(size_t)X.first[v] * 5 + 4] == 0.0f;
}
uint32_t gamma_key(const Example& X, int v) {
  return ((uint32_t)X.bpf_code[X.bpf_off[v]] << 16) | (uint32_t)(X.last[v] - X.first[v]);
}
// Phi rows: stem rows with one bp-frequency entry and no gap column whose
// children are all gamma rows.  Their G0 row is linear in per-y tables
// (dag_stem.hip): pf [sum_c w_c Phi_{code,len,key(c)} + xSL Gamma_{code,len}]
// + xwg sum_c w_c Gamma_{key(c)}, so the gamma schedule holds them as
// combination rows (no MATCH, no sweep).
bool is_phi(const Example& X, int v) {
  const uint32_t e0 = X.edge_off[v], e1 = X.edge_off[v + 1];
  if (e1 == e0 || 2 * (e1 - e0) + 1 > 255) return false;
  if (X.bpf_off[v + 1] - X.bpf_off[v] != 1 || X.prof5[(size_t)X.first[v] * 5 + 4] != 0.0f) return false;
  for (uint32_t k = e0; k < e1; ++k)
    if (!is_gamma(X, X.edge_to[k])) return false;
  return !is_gamma(X, v);
}

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

KeyTables key_tables(const std::vector<Example>& ex, int nthr) {
  KeyTables K;
  const int n = (int)ex.size();
  {  // every example's keys (host threads, one slice each), then one sorted set
    std::vector<std::vector<uint32_t>> tk(nthr);
    std::vector<std::vector<uint64_t>> tp(nthr);
    auto keys = [&](int t) {
      for (int e = (int)((int64_t)n * t / nthr); e < (int)((int64_t)n * (t + 1) / nthr); ++e) {
        const Example& X = ex[e];
        for (int v = 0; v < X.n_nodes(); ++v) {
          if (is_gamma(X, v)) tk[t].push_back(gamma_key(X, v));
          if (is_phi(X, v)) {
            tk[t].push_back(gamma_key(X, v));
            for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k)
              tp[t].push_back(((uint64_t)gamma_key(X, X.edge_to[k]) << 32) | gamma_key(X, v));
          }
        }
        auto& k1 = tk[t];  // keep each slice's lists short
        if (k1.size() > 4096) {
          std::sort(k1.begin(), k1.end());
          k1.erase(std::unique(k1.begin(), k1.end()), k1.end());
        }
        auto& p1 = tp[t];
        if (p1.size() > 4096) {
          std::sort(p1.begin(), p1.end());
          p1.erase(std::unique(p1.begin(), p1.end()), p1.end());
        }
      }
    };
    run_slices(nthr, keys);
    for (int t = 0; t < nthr; ++t) {
      K.gam_key.insert(K.gam_key.end(), tk[t].begin(), tk[t].end());
      K.phi_raw.insert(K.phi_raw.end(), tp[t].begin(), tp[t].end());
    }
  }
  std::sort(K.gam_key.begin(), K.gam_key.end());
  K.gam_key.erase(std::unique(K.gam_key.begin(), K.gam_key.end()), K.gam_key.end());
  K.gam_on = !K.gam_key.empty() && K.gam_key.size() <= 512 && !SK_KNOB("SK_NO_GAMMA");
  if (!K.gam_on) K.gam_key.clear();
  std::sort(K.phi_raw.begin(), K.phi_raw.end());
  K.phi_raw.erase(std::unique(K.phi_raw.begin(), K.phi_raw.end()), K.phi_raw.end());
  K.phi_on = K.gam_on && !K.phi_raw.empty() && K.phi_raw.size() < 0x4000 && !SK_KNOB("SK_NO_PHI");
  K.ss_on = K.gam_on && !SK_KNOB("SK_NO_SHARED_SUMS");
  if (const char* t = SK_KNOB("SK_SHARED_SUMS_THR")) K.ss_thr = std::atoi(t);
  return K;
}

// y-role records of one example (its nodes sorted by length, the IY sweep
// schedule, node-major edges), formed from its x-role arrays once the loop
// below has packed them: independent per example, so they run on host
// threads and are appended in example order (bit-identical to a serial pass)
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
  // the sweep chunks' SweepBanks cost in the plain order by length and as
  // packed, and whether the renumbering pass changed the order
  SweepCost cost_plain, cost;
  bool renumbered = false;
  long mg_plain = 0, mg_now = 0, mg_groups = 0;  // match_gather_cost of both orders (YOpts::stats)
  std::string err;
};
struct YOpts {
  bool sweep_lanes_greedy = true;
  bool renumber = true;  // renumber_equal_lengths (SK_NO_Y_RENUMBER=1: the plain stable order)
  bool stats = false;    // SK_PACK_STATS: the MATCH gather's read model too
};
void pack_y(const HostPack& P, const YOpts& opt, const YJob& J, YOut& Y) {
  const int nl = J.nl, ebase = J.ebase, bbase = J.bbase;
  const bool big = J.big;
  // y-role numbering for the stem kernel: nodes sorted by length (span
  // last - first), so the nodes inside a row's length band are one index
  // range and a node's children (strictly shorter) come before it; edges
  // grouped by parent level (the IY sweep walks levels) and contiguous per
  // parent, packed child:11 | parent:11 | gaps:10 in sorted ids.  The order
  // inside a run of equal lengths is free: renumber_equal_lengths chooses it
  // once the chunks are composed, for a second set of the records (Y.r; the
  // big-y path keeps the plain order there too).
  {
    std::vector<int> srt(nl);
    std::iota(srt.begin(), srt.end(), 0);
    auto len_of = [&](int k) { return P.nd_b[J.nb0 + k] & 0xffff; };
    std::stable_sort(srt.begin(), srt.end(), [&](int a, int b) { return len_of(a) < len_of(b); });
    std::vector<int> pos(nl);
    for (int i = 0; i < nl; ++i) pos[srt[i]] = i;
    const int nb0 = J.nb0;
    std::vector<int> srt_r, pos_r;  // the renumbered order (Y.r)
    // IY sweep schedule.  The sweep is a stream of chunks of 64 edges: a
    // chunk's R[child] reads are issued after the previous chunk's
    // atomics, so an edge may go into any chunk after the one holding the
    // last edge of its child (every node's value is final by then).  List
    // scheduling, priority = height of the parent (longest path up to a
    // root; the critical chain first), then the child's length; chunks
    // are padded with dummy records (child == parent: weight 0).
    if (big) {  // no sweep schedule: the big-y kernel walks the levels
      const int lmax = nl ? (int)(P.nd_b[nb0 + srt[nl - 1]] & 0xffff) : 0;
      for (int v = 0; v <= lmax + 1; ++v) Y.ycs.push_back(0);
      Y.nch = 0;
    } else {
      SweepSchedule S;
      S.nl = nl;
      S.lanes_greedy = opt.sweep_lanes_greedy;
      std::vector<uint32_t>& er = S.er;  // records child:11 | parent:11 | gaps:10
      std::vector<int>&epar = S.epar, &ech = S.ech;
      for (int k = 0; k < nl; ++k) {
        const uint32_t a = P.nd_a[nb0 + k];
        const uint32_t ne = (a >> 16) & 0xff, el = a & 0xffff;
        for (uint32_t t = 0; t < ne; ++t) {
          const uint2 rec = P.ed[ebase + el + t];  // {child | gaps<<16, parent}
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
      std::vector<int32_t> cm;  // prefix maximum of the children's lengths
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
      if (placed != ne_all) {
        Y.err = "IY sweep schedule: DAG has a cycle";
        return;
      }
      const int nch = (int)cm.size();
      // the chunks are composed: their records dealt to the lanes in the
      // plain order, then in the order renumber_equal_lengths chooses inside
      // the runs of equal length
      auto emit_lanes = [&](const std::vector<uint32_t>& recs, YRec& A) {
        SweepCost dealt;
        for (int c = 0; c < nch; ++c) {
          uint32_t lanes[64];
          int rd, at;
          sweep_chunk_lanes(S.chunk_ed.data() + S.chunk_off[c], S.chunk_off[c + 1] - S.chunk_off[c], recs, nl,
                            opt.sweep_lanes_greedy, lanes);
          sweep_chunk_cost(lanes, &rd, &at);
          dealt.read += rd;
          dealt.atomic += at;
          A.ysc.insert(A.ysc.end(), lanes, lanes + 64);
        }
        return dealt;
      };
      Y.cost_plain = Y.cost = emit_lanes(er, Y);
      if (opt.renumber) {
        std::vector<int> len(nl), newid;
        for (int i = 0; i < nl; ++i) len[i] = (int)(P.nd_b[nb0 + srt[i]] & 0xffff);
        renumber_equal_lengths(S, len, newid, Y.cost_plain, Y.cost);
        for (int i = 0; i < nl && !Y.renumbered; ++i) Y.renumbered = newid[i] != i;
        if (Y.renumbered) {
          srt_r.resize(nl);
          pos_r.resize(nl);
          for (int i = 0; i < nl; ++i) srt_r[newid[i]] = srt[i];
          for (int i = 0; i < nl; ++i) pos_r[srt_r[i]] = i;
          for (uint32_t& r : er)
            r = (r & ~0x3fffffu) | (uint32_t)newid[r & 0x7ff] | ((uint32_t)newid[(r >> 11) & 0x7ff] << 11);
          emit_lanes(er, Y.r);
        } else {
          Y.r.ysc = Y.ysc;
        }
      }
      // first chunk whose prefix maximum reaches v, v = 0 .. lmax+1
      const int lmax = nl ? (int)(P.nd_b[nb0 + srt[nl - 1]] & 0xffff) : 0;
      for (int v = 0, c = 0; v <= lmax + 1; ++v) {
        while (c < nch && cm[c] < v) ++c;
        Y.ycs.push_back(c);
      }
      Y.nch = nch;
    }
    // node-major copy of the edges in sorted order (the MATCH sums of a
    // run of consecutive nodes read one contiguous edge range); a node's
    // record keeps its first edge there, E(q) = prefix sum of n_edges
    auto emit_nodes = [&](const std::vector<int>& srt, const std::vector<int>& pos, YRec& Y) {
    const int ye2_base = (int)Y.ye2.size();
    for (int i = 0; i < nl; ++i) {
      const int k = srt[i];
      Y.src.push_back((uint32_t)k);
      const uint32_t a = P.nd_a[nb0 + k];
      const uint32_t ne = (a >> 16) & 0xff, el = a & 0xffff;
      const uint32_t nbf = a >> 24, bl = P.nd_b[nb0 + k] >> 16;
      Y.yn_a.push_back(((uint32_t)Y.ye2.size() - ye2_base) | (a & 0xffff0000u));
      for (uint32_t t = 0; t < ne; ++t) {
        const uint2 rec = P.ed[ebase + el + t];
        Y.ye2.push_back(big ? 0u : (uint32_t)pos[rec.x & 0xffff] | ((uint32_t)i << 11) |
                                       ((rec.x >> 16) << 22));
      }
      // c = loop leaf-edge gaps:16 | first bp-freq code:4 | single-entry flag
      // (one bp-freq entry, no gap column: the closed-form node score)
      const bool one = nbf == 1 && P.nd_nbp[nb0 + k] == 0.0f;
      const uint32_t bc0 = nbf ? P.bpf_code[bbase + bl] & 0xf : 0u;
      Y.yn_c.push_back((P.nd_c[nb0 + k] & 0xffff) | (bc0 << 16) | ((one ? 1u : 0u) << 24));
      Y.yn_p0.push_back(nbf ? P.bpf_p[bbase + bl] : 0.0f);
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
    };
    emit_nodes(srt, pos, Y);
    if (opt.renumber) emit_nodes(Y.renumbered ? srt_r : srt, Y.renumbered ? pos_r : pos, Y.r);
    if (opt.stats && opt.renumber && !big) {  // the MATCH gather's reads in both orders, from every length's first edge
      std::vector<int> starts;
      std::vector<uint32_t> now, plain;
      for (int i = 0; i < nl; ++i)
        if (i == 0 || (Y.yn_b[i] & 0xffff) != (Y.yn_b[i - 1] & 0xffff)) starts.push_back((int)(Y.yn_a[i] & 0xffff));
      for (uint32_t e : Y.r.ye2) now.push_back(e & 0x7ff);
      for (uint32_t e : Y.ye2) plain.push_back(e & 0x7ff);
      long g2 = 0;
      match_gather_cost(now, starts, &Y.mg_now, &Y.mg_groups);
      match_gather_cost(plain, starts, &Y.mg_plain, &g2);
    }
  }
}

// x-role records of one example (nodes in level order, the x schedules,
// per-position tables), formed per example on host threads and appended
// in example order below (bit-identical to one serial pass; example-local
// offsets, the dataset's bases added when appending)
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
void pack_x(const Example& X, const KeyTables& K, XOut& O) {
  const int nn = X.n_nodes();
  // level of every node (children first in reference numbering)
  std::vector<int> level(nn, -1);
  int nlev = 0;
  for (int v = 0; v < nn; ++v) {
    const uint32_t e0 = X.edge_off[v], e1 = X.edge_off[v + 1];
    if (e0 == e1) continue;  // leaf
    int lv = 0;
    bool any_leaf = false;
    for (uint32_t k = e0; k < e1; ++k) {
      const int c = level[X.edge_to[k]];
      if (c < 0) any_leaf = true;
      else lv = std::max(lv, c + 1);
    }
    if (any_leaf && e1 - e0 != 1) {
      O.err = "unexpected DAG shape: stem with a leaf child";
      O.rc = SK_ERR_INVALID;
      return;
    }
    level[v] = lv;
    nlev = std::max(nlev, lv + 1);
  }
  std::vector<int> order;  // non-leaf nodes by (level, reference index): a counting sort
  {
    std::vector<int> lstart(nlev + 1, 0);
    for (int v = 0; v < nn; ++v)
      if (level[v] >= 0) ++lstart[level[v] + 1];
    for (int l = 0; l < nlev; ++l) lstart[l + 1] += lstart[l];
    order.resize(lstart[nlev]);
    for (int v = 0; v < nn; ++v)
      if (level[v] >= 0) order[lstart[level[v]]++] = v;
  }
  const int nl = (int)order.size();
  if (nl >= 0xffff) {
    O.err = "example too large: more than 65534 non-leaf DAG nodes";
    O.rc = SK_ERR_UNSUPPORTED;
    return;
  }
  std::vector<int> nid(nn, -1);
  for (int k = 0; k < nl; ++k) nid[order[k]] = k;
  // per-node gamma (bit 0) / phi (bit 1) row flags, tested once here: the
  // passes below ask repeatedly
  // and their (code, len) key's index (looked up once per node)
  std::vector<uint8_t> fl(nn, 0);
  std::vector<uint32_t> gix(nn, 0);
  if (K.gam_on)
    for (int v = 0; v < nn; ++v) fl[v] |= is_gamma(X, v) ? 1 : 0;
  if (K.phi_on)
    for (int v = 0; v < nn; ++v) fl[v] |= is_phi(X, v) ? 2 : 0;
  for (int v = 0; v < nn; ++v)
    if (fl[v]) gix[v] = K.gamma_idx(gamma_key(X, v));
  {
    const size_t ne_x = (size_t)X.n_edges();
    for (auto* q : {&O.nd_a, &O.nd_b, &O.nd_c, &O.xr_node, &O.xg_node}) q->reserve(nl);
    O.nd_w.reserve(nl);
    O.nd_nbp.reserve(nl);
    O.nd_P.reserve(nl);
    O.ed.reserve(ne_x);
    O.xr_ch.reserve(ne_x);
    O.xrow.reserve(nl);
    O.xgrow.reserve(nl);
    O.xg_ch.reserve(2 * ne_x + nl);
    O.xg_clg.reserve(2 * ne_x + nl);
    O.xg_cpf.reserve(2 * ne_x + nl);
    O.xg_cty.reserve(2 * ne_x + nl);
    O.bpf_code.reserve(X.bpf_off[nn]);
    O.bpf_p.reserve(X.bpf_off[nn]);
  }
  // path weights: number of root->v paths (parents have larger reference ids)
  std::vector<double> Pw(nn, 0.0);
  for (uint32_t r : X.roots) Pw[r] += 1.0;
  for (int v = nn - 1; v >= 0; --v)
    for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k) Pw[X.edge_to[k]] += Pw[v];


  bool big_gap = false;
  for (int k = 0; k < nl; ++k) {
    const int v = order[k];
    const uint32_t e0 = X.edge_off[v], e1 = X.edge_off[v + 1];
    const uint32_t b0 = X.bpf_off[v], b1 = X.bpf_off[v + 1];
    const bool loop = level[v] == 0;  // single leaf child
    const uint32_t eloc = (uint32_t)O.ed.size(), bloc = (uint32_t)O.bpf_code.size();
    const uint32_t ne = loop ? 0u : e1 - e0;
    if (eloc > 0xffff || bloc > 0xffff || ne > 0xff || b1 - b0 > 0xff ||
        X.last[v] - X.first[v] > 0xffff) {
      O.err = "example too large for the 16-bit packed DAG layout";
      O.rc = SK_ERR_UNSUPPORTED;
      return;
    }
    O.nd_a.push_back(eloc | (ne << 16) | ((b1 - b0) << 24));
    O.nd_b.push_back((X.last[v] - X.first[v]) | (bloc << 16));
    O.nd_c.push_back(loop ? X.edge_gaps[e0] : 0u);
    O.nd_w.push_back(X.weight[v]);
    O.nd_nbp.push_back(X.prof5[(size_t)X.first[v] * 5 + 4]);
    O.nd_P.push_back(Pw[v]);
    if (!loop) {
      for (uint32_t t = e0; t < e1; ++t) {
        const int c = nid[X.edge_to[t]];
        if (c < 0 || X.edge_gaps[t] > 0xffff) {
          O.err = c < 0 ? "unexpected DAG shape: stem with a leaf child" : "gap count exceeds 65535";
          O.rc = c < 0 ? SK_ERR_INVALID : SK_ERR_UNSUPPORTED;
          return;
        }
        big_gap |= X.edge_gaps[t] > 1023;
        O.ed.push_back(make_uint2((uint32_t)c | (X.edge_gaps[t] << 16), (uint32_t)k));
      }
    }
    for (uint32_t t = b0; t < b1; ++t) {
      O.bpf_code.push_back(X.bpf_code[t]);
      O.bpf_p.push_back(X.bpf_p[t]);
    }
  }
  std::vector<int32_t> lv(nlev + 1, 0);
  for (int k = 0; k < nl; ++k) lv[level[order[k]] + 1]++;
  for (int l = 0; l < nlev; ++l) lv[l + 1] += lv[l];
  O.lvl.insert(O.lvl.end(), lv.begin(), lv.end());
  // the register-class kernel's y records: child:11 | parent:11 | gaps:10
  // (at most 2,047 nodes: every register class keeps its last slot free,
  // the dummy records' target, dag_stem.hip)
  const bool big = nl > 2047 || big_gap;
  O.ex_big.push_back(big ? 1 : 0);

  // (the y-role records are formed after the x-role pass: pack_y below)
  O.nl = nl;
  O.big = big;

  // x-role schedule: rows in reference (post-)order; a row's HBM slot is
  // recycled once its last parent has been produced (LIFO free list keeps
  // hot addresses hot).  Rows nobody reads (roots) get no slot.
  {
    std::vector<int> last_parent(nn, -1);
    for (int v = 0; v < nn; ++v)
      for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k)
        last_parent[X.edge_to[k]] = std::max(last_parent[X.edge_to[k]], v);
    std::vector<uint32_t> slot(nn, 0xffff);
    std::vector<int> free_list;
    int nslots = 0;
    for (int v = 0; v < nn; ++v) {
      if (level[v] < 0) continue;
      const bool loop = level[v] == 0;
      const uint32_t e0 = X.edge_off[v], e1 = X.edge_off[v + 1];
      const uint32_t b0 = X.bpf_off[v], b1 = X.bpf_off[v + 1];
      uint32_t nch = 0;
      if (!loop) {
        for (uint32_t k = e0; k < e1; ++k) {
          const int c = X.edge_to[k];
          O.xr_ch.push_back(slot[c] | (X.edge_gaps[k] << 16));
          ++nch;
        }
      }
      for (uint32_t k = e0; k < e1; ++k) {
        const int c = X.edge_to[k];
        if (level[c] >= 0 && last_parent[c] == v && slot[c] != 0xffff) free_list.push_back(slot[c]);
      }
      if (last_parent[v] >= 0) {
        int sl;
        if (!free_list.empty()) {
          sl = free_list.back();
          free_list.pop_back();
        } else {
          sl = nslots++;
        }
        slot[v] = (uint32_t)sl;
      }
      sk::XRow xr;
      xr.a = nch | ((b1 - b0) << 8) | ((loop ? X.edge_gaps[e0] : 0u) << 16);
      xr.b = (X.last[v] - X.first[v]) | (slot[v] << 16);
      xr.w = X.weight[v];
      xr.nbp = X.prof5[(size_t)X.first[v] * 5 + 4];
      xr.bp0 = b1 > b0 ? X.bpf_p[b0] : 0.0f;
      xr.P = Pw[v];
      // bpf_beg in the level-order bpf array of this example (see nd_b)
      xr.c = (O.nd_b[nid[v]] >> 16) | ((b1 > b0 ? (uint32_t)X.bpf_code[b0] : 0u) << 16);
      O.xrow.push_back(xr);
      O.xr_node.push_back((uint32_t)nid[v]);
    }
    if (nslots >= 0xffff) {
      O.err = "too many live DAG rows";
      O.rc = SK_ERR_UNSUPPORTED;
      return;
    }
    O.ex_nslots.push_back(nslots);
    O.max_slots = std::max(O.max_slots, nslots);

    // the gamma schedule: the same post-order without the gamma rows
    // (slots only among the remaining rows; a gamma child is a record
    // 0x8000 | gamma index, its weight factors g^lg pf in xg_clg / xg_cpf)
    std::vector<uint32_t> gslot(nn, 0xffff);
    std::vector<int> gfree;
    int gslots = 0, nlxg = 0;
    // row order: a depth-first post-order whose last-visited child of a
    // row is, where it can be, one that row alone reads among its first
    // four records (stored nowhere: the row takes it from registers; see
    // below), the reference numbering with SK_REF_ORDER; then each phi row
    // moved to just before its first parent (it has no row children, so
    // any earlier place is valid): the parent takes it from registers too
    // (distance 1), and the row before it, usually a swept one, prefetches
    // its first components
    std::vector<int> order;
    {
      std::vector<int> npar(nn, 0), cand(nn, -1);
      for (int v = 0; v < nn; ++v)
        for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k) ++npar[X.edge_to[k]];
      for (int v = 0; v < nn; ++v) {
        if (level[v] <= 0 || (fl[v] & 2)) continue;
        for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1] && k < X.edge_off[v] + 4; ++k) {
          const int c = X.edge_to[k];
          if (npar[c] == 1 && level[c] >= 0 && !(fl[c] & 1)) {
            cand[v] = c;
            break;
          }
        }
      }
      if (SK_KNOB("SK_REF_ORDER")) {
        for (int v = 0; v < nn; ++v)
          if (level[v] >= 0) order.push_back(v);
      } else {
        std::vector<uint8_t> seen(nn, 0);
        std::vector<std::pair<int, int>> st;  // (row, next child index; -1: candidate done)
        auto dfs = [&](int s) {
          if (seen[s] || level[s] < 0) return;
          seen[s] = 1;
          st.push_back({s, 0});
          while (!st.empty()) {
            auto& [v, i] = st.back();
            const int ne = (int)(X.edge_off[v + 1] - X.edge_off[v]);
            int next = -1;
            while (i >= 0 && i < ne && next < 0) {
              const int c = X.edge_to[X.edge_off[v] + i++];
              if (c != cand[v] && !seen[c] && level[c] >= 0) next = c;
            }
            if (next < 0 && i >= 0) {
              i = -1;
              if (cand[v] >= 0 && !seen[cand[v]]) next = cand[v];
            }
            if (next < 0) {
              order.push_back(v);
              st.pop_back();
            } else {
              seen[next] = 1;
              st.push_back({next, 0});
            }
          }
        };
        for (uint32_t r : X.roots) dfs((int)r);
        for (int v = nn - 1; v >= 0; --v) dfs(v);
      }
      std::vector<int> pos(nn, nn), first_parent(nn, nn);
      for (int i = 0; i < (int)order.size(); ++i) pos[order[i]] = i;
      for (int v = 0; v < nn; ++v)
        for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k) {
          const int c = X.edge_to[k];
          if (pos[v] < nn && (first_parent[c] == nn || pos[v] < pos[first_parent[c]])) first_parent[c] = v;
        }
      // the phi rows moved before each row (first parent nn: the roots'),
      // in order, as one CSR list
      const bool move = K.phi_on && !SK_KNOB("SK_PHI_POSTORDER");
      std::vector<int> o1, boff(nn + 2, 0), bl;
      o1.reserve(order.size());
      for (int v : order) {
        if (move && (fl[v] & 2)) ++boff[first_parent[v] + 1];
        else o1.push_back(v);
      }
      for (int i = 0; i <= nn; ++i) boff[i + 1] += boff[i];
      bl.resize(boff[nn + 1]);
      {
        std::vector<int> bf(boff.begin(), boff.end() - 1);
        for (int v : order)
          if (move && (fl[v] & 2)) bl[bf[first_parent[v]]++] = v;
      }
      std::vector<int> o2;
      o2.reserve(order.size() + 8);
      for (int v : o1) {
        const auto bb = bl.begin() + boff[v], be = bl.begin() + boff[v + 1];
        const auto it = std::find(bb, be, cand[v]);
        if (it != be) {
          std::rotate(it, it + 1, be);  // the candidate last
          o2.insert(o2.end(), bb, be);
        } else if (bb != be && cand[v] >= 0 && !o2.empty() && o2.back() == cand[v]) {
          o2.pop_back();
          o2.insert(o2.end(), bb, be);
          o2.push_back(cand[v]);
        } else {
          o2.insert(o2.end(), bb, be);
        }
        o2.push_back(v);
      }
      o2.insert(o2.end(), bl.begin() + boff[nn], bl.begin() + boff[nn + 1]);  // roots
      order.swap(o2);
    }
    // each row's slot is freed at its last parent in this order
    std::vector<int> glast(nn, -1);
    {
      std::vector<int> gpos(nn, -1);
      for (int i = 0; i < (int)order.size(); ++i) gpos[order[i]] = i;
      for (int v : order)
        for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k) {
          const int c = X.edge_to[k];
          if (glast[c] < 0 || gpos[v] > gpos[glast[c]]) glast[c] = v;
        }
    }
    // rows read only by the next row, among its first four children, are
    // never stored: the next row takes them from registers (slot 0xfffe)
    std::vector<uint8_t> nostore(nn, 0);
    if (!SK_KNOB("SK_STORE_ALL")) {
      std::vector<int> npar(nn, 0), emitted;
      for (int v = 0; v < nn; ++v)
        for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k) ++npar[X.edge_to[k]];
      for (int v : order)
        if (!(fl[v] & 1)) emitted.push_back(v);
      for (size_t i = 0; i + 1 < emitted.size(); ++i) {
        const int v = emitted[i], r = emitted[i + 1];
        if (npar[v] != 1 || level[r] <= 0 || level[v] < 0 || (fl[r] & 2)) continue;
        for (uint32_t k = X.edge_off[r]; k < X.edge_off[r + 1] && k < X.edge_off[r] + 4; ++k)
          if (X.edge_to[k] == v) nostore[v] = 1;
      }
    }
    // the same rows as the input of the factored schedule
    std::vector<sk::SsRow> ss_in;
    std::vector<int32_t> grow_of(nn, -1);
    std::vector<uint32_t> ss_gra;  // the phi rows, by input row
    if (K.ss_on) ss_in.reserve(order.size());
    uint32_t ss_key = (uint32_t)nn;  // identities of the phi rows' components (never shared)
    for (int v : order) {
      const uint32_t e0 = X.edge_off[v], e1 = X.edge_off[v + 1];
      const uint32_t b0 = X.bpf_off[v], b1 = X.bpf_off[v + 1];
      if (fl[v] & 1) {
        O.gr_info.push_back(gix[v] | (X.edge_gaps[e0] << 16));
        O.gr_pf.push_back(X.bpf_p[b0]);
        O.gr_P.push_back(Pw[v]);
        continue;
      }
      const bool loop = level[v] == 0;
      const bool phi = (fl[v] & 2) != 0;
      uint32_t nch = 0;
      const size_t rec0 = O.xg_ch.size();
      if (phi) {
        // components: per child c a Phi row (type 2) and its Gamma row
        // (type 4), then Gamma_{code,len} of the row itself (type 3)
        const uint32_t kp = gamma_key(X, v);
        for (uint32_t k = e0; k < e1; ++k) {
          const int c = X.edge_to[k];
          const uint32_t kc = gamma_key(X, c);
          const uint32_t pi = K.phi_idx(kp, kc);
          for (int ty : {2, 4}) {
            O.xg_ch.push_back(((ty == 2 ? 0x4000u | pi : 0x8000u | gix[c])) | (X.edge_gaps[k] << 16));
            O.xg_clg.push_back(X.edge_gaps[X.edge_off[c]]);
            O.xg_cpf.push_back(X.bpf_p[X.bpf_off[c]]);
            O.xg_cty.push_back((uint8_t)ty);
          }
          O.phk_idx.push_back(pi);
        }
        O.xg_ch.push_back(0x8000u | gix[v]);
        O.xg_clg.push_back(0u);
        O.xg_cpf.push_back(0.0f);
        O.xg_cty.push_back(3);
        O.gra_gidx.push_back(gix[v]);
        O.gra_row.push_back((uint32_t)O.xgrow.size());  // (+ the example's xgrow base)
        nch = 2 * (e1 - e0) + 1;
      } else if (!loop) {
        for (uint32_t k = e0; k < e1; ++k) {
          const int c = X.edge_to[k];
          if (fl[c] & 1) {
            O.xg_ch.push_back((0x8000u | gix[c]) | (X.edge_gaps[k] << 16));
            O.xg_clg.push_back(X.edge_gaps[X.edge_off[c]]);
            O.xg_cpf.push_back(X.bpf_p[X.bpf_off[c]]);
            O.xg_cty.push_back(1);
          } else {
            O.xg_ch.push_back(gslot[c] | (X.edge_gaps[k] << 16));
            O.xg_clg.push_back(0u);
            O.xg_cpf.push_back(1.0f);
            O.xg_cty.push_back(0);
          }
          ++nch;
        }
      }
      for (uint32_t k = e0; k < e1; ++k) {
        const int c = X.edge_to[k];
        if (level[c] >= 0 && glast[c] == v && gslot[c] < 0x4000) {
          gfree.push_back(gslot[c]);
          gslot[c] |= 0x10000;  // freed (a second edge to c must not free it again)
        }
      }
      if (nostore[v]) {
        gslot[v] = 0xfffe;
      } else if (last_parent[v] >= 0) {
        int sl;
        if (!gfree.empty()) {
          sl = gfree.back();
          gfree.pop_back();
        } else {
          sl = gslots++;
        }
        gslot[v] = (uint32_t)sl;
      }
      sk::XRow xr;
      xr.a = nch | ((b1 - b0) << 8) | ((loop ? X.edge_gaps[e0] : 0u) << 16);
      xr.b = (X.last[v] - X.first[v]) | (gslot[v] << 16);
      xr.w = X.weight[v];
      xr.nbp = X.prof5[(size_t)X.first[v] * 5 + 4];
      xr.bp0 = b1 > b0 ? X.bpf_p[b0] : 0.0f;
      xr.P = Pw[v];
      xr.c = (O.nd_b[nid[v]] >> 16) | ((b1 > b0 ? (uint32_t)X.bpf_code[b0] : 0u) << 16) |
             (phi ? 0x80000000u : 0u);
      if (K.ss_on) {
        sk::SsRow W;
        W.xr = xr;
        W.node = (uint32_t)nid[v];
        W.user = W.swept = !phi && !loop;
        size_t t = rec0;
        auto table = [&](uint32_t key) {
          W.rec.push_back(sk::SsRec{-1, key, O.xg_ch[t] & 0xffffu, O.xg_ch[t] >> 16, O.xg_clg[t], O.xg_cpf[t],
                                    O.xg_cty[t]});
          ++t;
        };
        if (phi) {
          for (; t < O.xg_ch.size();) table(ss_key++);
          ss_gra.push_back((uint32_t)O.xgrow.size());
        } else if (!loop) {
          for (uint32_t k = e0; k < e1; ++k) {
            const int c = X.edge_to[k];
            if (fl[c] & 1) {
              table((uint32_t)c);
            } else {
              W.rec.push_back(sk::SsRec{grow_of[c], 0u, 0u, X.edge_gaps[k], 0u, 1.0f, 0});
              ++t;
            }
          }
        }
        grow_of[v] = (int32_t)O.xgrow.size();
        ss_in.push_back(std::move(W));
      }
      O.xgrow.push_back(xr);
      O.xg_node.push_back((uint32_t)nid[v]);
      ++nlxg;
    }
    if (K.ss_on) {
      sk::SsOut F;
      if (sk::shared_sums_schedule(std::move(ss_in), K.ss_thr, SK_KNOB("SK_STORE_ALL") != nullptr, F)) {
        O.xf_row.swap(F.row);
        O.xf_node.swap(F.node);
        O.xf_ch.swap(F.ch);
        O.xf_clg.swap(F.clg);
        O.xf_cpf.swap(F.cpf);
        O.xf_cty.swap(F.cty);
        for (uint32_t r : ss_gra) O.xf_gra_row.push_back(F.new_index[r]);  // (+ the example's base)
        O.ss_rows = F.n_shared;
        O.ss_repl = F.n_replaced;
        O.max_slots = std::max(O.max_slots, F.nslots);
      } else {  // over a limit of the layout: this example keeps its plain rows
        O.xf_row = O.xgrow;
        O.xf_node = O.xg_node;
        O.xf_ch = O.xg_ch;
        O.xf_clg = O.xg_clg;
        O.xf_cpf = O.xg_cpf;
        O.xf_cty = O.xg_cty;
        O.xf_gra_row = O.gra_row;
      }
    }
    if (K.phi_on) {  // this example's phi keys as a bitset (items take unions)
      const size_t W = (K.phi_raw.size() + 63) / 64;
      O.ex_phi_bits.assign(W, 0ull);
      for (size_t j = 0; j < O.phk_idx.size(); ++j)
        O.ex_phi_bits[O.phk_idx[j] / 64] |= 1ull << (O.phk_idx[j] % 64);
    }
    if (gslots >= 0x4000) {  // slot ids share the record with the gamma / phi flags
      O.err = "too many live DAG rows";
      O.rc = SK_ERR_UNSUPPORTED;
      return;
    }
    O.ex_nlxg.push_back(nlxg);
    O.max_slots = std::max(O.max_slots, gslots);
    O.n_nostore = 0;
    for (int v = 0; v < nn; ++v) O.n_nostore += nostore[v];
    O.n_nodes = nn;
    O.gslots = gslots;
  }
  {  // y role: no gap column in any non-leaf node (the Gamma rows need it)
    bool gl = true;
    for (int k = 0; k < nl; ++k) gl &= O.nd_nbp[k] == 0.0f;
    O.ex_gapless.push_back(gl ? 1 : 0);
  }
  O.ex_nl.push_back(nl);
  O.ex_nlev.push_back(nlev);
  O.nlev = nlev;
  O.ex_nseqs.push_back(X.n_seqs);
  O.ex_len.push_back(X.len);
  O.ex_has_w.push_back(X.has_bp ? 1 : 0);
  for (int i = 0; i < X.len; ++i) {
    const float* c = &X.prof5[(size_t)i * 5];
    O.pos_prof.push_back(make_float4(c[0], c[1], c[2], c[3]));
    O.pos_w.push_back(X.has_bp ? X.pos_weight[i] : 1.0f);
    O.pos_chr.push_back((uint8_t)X.rows[0][i]);
  }
  bpla_weights(X, O.pos_lru);
  {
    bool dy = true;  // the device's dyadic_sum test (bpla.hip), in host float
    for (int i = 0; i < X.len; ++i)
      for (int k = 0; k < 4; ++k) {
        const float v = X.prof5[(size_t)i * 5 + k] * 256.0f;
        dy = dy && v == std::rint(v);
      }
    O.ex_dyadic.push_back(dy ? 1 : 0);
    bool full = true;
    for (int i = 0; i < X.len; ++i) {
      const float* c = &X.prof5[(size_t)i * 5];
      full = full && (c[0] + c[1] + c[2] + c[3]) > 0.0f;
    }
    O.ex_str_fast.push_back(dy && full ? 1 : 0);
    bool oh = true;  // the device's onehot_code test (profile_string.hip)
    for (int i = 0; i < X.len && oh; ++i) {
      const float* c = &X.prof5[(size_t)i * 5];
      int ones = 0, zeros = 0;
      for (int k = 0; k < 4; ++k) {
        ones += c[k] == 1.0f;
        zeros += c[k] == 0.0f;
      }
      oh = ones == 1 && zeros == 3;
    }
    O.ex_onehot.push_back(oh ? 1 : 0);
  }
}

}  // namespace

// BPLA fill_weight (bpla_kernel/data.cpp:19-45) over the averaged bp matrix:
// float accumulators with each add rounded from double, then sqrt.
float4 bpla_weight(const Example& X, int i) {
  if (!X.has_bp) return make_float4(0.f, 0.f, 1.f, 0.f);
  float pl = 0.0f, pr = 0.0f;
  for (int j = 0; j < i; ++j) pr = (float)((double)pr + X.bpp[sk::tri_index(X.len, j, i)]);
  for (int j = i + 1; j < X.len; ++j) pl = (float)((double)pl + X.bpp[sk::tri_index(X.len, i, j)]);
  float pu = (float)(1.0 - (double)(pl + pr));
  if (pu < 0.0f) pu = 0.0f;
  return make_float4(std::sqrt(pl), std::sqrt(pr), std::sqrt(pu), 0.f);
}

// --------------------------------------------------------------- packing
int pack_dataset(sk_dataset* ds, std::string& err, const std::function<void()>* after_x) {
  HostPack& P = ds->pack;
  const bool tstats = std::getenv("SK_HOST_STATS") != nullptr;
  auto tnow = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double tp0 = tnow();
  // SK_SWEEP_LANES=0: sweep chunks in schedule order (A/B diagnostics)
  const char* lanes_env = SK_KNOB("SK_SWEEP_LANES");
  const bool sweep_lanes_greedy = !lanes_env || std::atoi(lanes_env) != 0;
  P = HostPack();
  const int n = (int)ds->ex.size();
  // host threads of the packing passes (SK_PACK_THREADS caps them: the
  // packed arrays do not depend on it, tests/test_pack_threads.py)
  const size_t pcap = std::getenv("SK_PACK_THREADS") ? (size_t)std::max(1, std::atoi(std::getenv("SK_PACK_THREADS")))
                                                     : (size_t)16;
  const int nthr = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n / 8 + 1, pcap,
                                                              (size_t)std::max(1u, std::thread::hardware_concurrency())}));
  const KeyTables K = key_tables(ds->ex, nthr);
  P.gam_key = K.gam_key;
  P.shared_sums = K.ss_on;
  if (K.phi_on)
    for (uint64_t k : K.phi_raw) {
      P.phi_al.push_back((uint32_t)k);
      P.phi_g.push_back(K.gamma_idx((uint32_t)(k >> 32)));
    }
  std::vector<YJob> yjobs;
  yjobs.reserve(n);
  const double tp1 = tnow();
  double tpx = tp1;
  {
    std::vector<XOut> xo(n);
    std::atomic<int> next{0};
    auto work = [&]() {
      for (int e = next.fetch_add(1); e < n; e = next.fetch_add(1)) pack_x(ds->ex[e], K, xo[e]);
    };
    run_pool(nthr, work);
    tpx = tnow();
    P.ex_node_base.push_back(0);
    P.ex_edge_base.push_back(0);
    P.ex_bpf_base.push_back(0);
    P.ex_lvl_base.push_back(0);
    P.ex_pos_base.push_back(0);
    // per-example arrays at their prefix-sum offsets, copied on the threads
#define SK_BIG(X) X(nd_a) X(nd_b) X(nd_c) X(nd_w) X(nd_nbp) X(nd_P) X(ed) X(bpf_code) X(bpf_p) X(lvl) \
  X(xr_ch) X(xrow) X(xr_node) X(gr_info) X(gr_pf) X(gr_P) X(xg_ch) X(xg_clg) X(xg_cpf) X(xg_cty)    \
  X(phk_idx) X(gra_gidx) X(gra_row) X(xgrow) X(xg_node) X(pos_prof) X(pos_w) X(pos_chr) X(pos_lru)  \
  X(ex_phi_bits) X(xf_row) X(xf_node) X(xf_ch) X(xf_clg) X(xf_cpf) X(xf_cty) X(xf_gra_row)
#define SK_OFF(f) std::vector<size_t> off_##f(n + 1, 0);
    SK_BIG(SK_OFF)
#undef SK_OFF
    auto app = [](auto& dst, const auto& src) { dst.insert(dst.end(), src.begin(), src.end()); };
    std::vector<long> st_nodes(n), st_nost(n), st_slots(n);  // (SK_PACK_STATS)
    for (int e = 0; e < n; ++e) {
      XOut& O = xo[e];
      st_nodes[e] = O.n_nodes;
      st_nost[e] = O.n_nostore;
      st_slots[e] = O.gslots;
      if (O.rc) {  // the first failing example, as the serial pass would report it
        err = O.err;
        return O.rc;
      }
#define SK_ACC(f) off_##f[e + 1] = off_##f[e] + O.f.size();
      SK_BIG(SK_ACC)
#undef SK_ACC
      yjobs.push_back(YJob{(int)off_nd_a[e], (int)off_ed[e], (int)off_bpf_code[e], O.nl, O.big});
      P.ex_xch_base.push_back((int32_t)off_xr_ch[e]);
      P.ex_xg_base.push_back((int32_t)off_xgrow[e]);
      P.ex_xgch_base.push_back((int32_t)off_xg_ch[e]);
      P.ex_gr_base.push_back((int32_t)off_gr_info[e]);
      P.ex_gra_base.push_back((int32_t)off_gra_gidx[e]);
      P.ex_phk_base.push_back((int32_t)off_phk_idx[e]);
      if (K.ss_on) {
        P.ex_xf_base.push_back((int32_t)off_xf_row[e]);
        P.ex_xfch_base.push_back((int32_t)off_xf_ch[e]);
        P.ex_nlxf.push_back((int32_t)O.xf_row.size());
        P.ex_ss_rows.push_back(O.ss_rows);
        P.ex_ss_repl.push_back(O.ss_repl);
      }
      app(P.ex_big, O.ex_big); app(P.ex_nslots, O.ex_nslots); app(P.ex_nlxg, O.ex_nlxg);
      app(P.ex_gapless, O.ex_gapless); app(P.ex_nl, O.ex_nl); app(P.ex_nlev, O.ex_nlev);
      app(P.ex_nseqs, O.ex_nseqs); app(P.ex_len, O.ex_len); app(P.ex_has_w, O.ex_has_w);
      app(P.ex_dyadic, O.ex_dyadic); app(P.ex_str_fast, O.ex_str_fast); app(P.ex_onehot, O.ex_onehot);
      P.max_slots = std::max(P.max_slots, O.max_slots);
      P.ex_node_base.push_back((int32_t)off_nd_a[e + 1]);
      P.ex_edge_base.push_back((int32_t)off_ed[e + 1]);
      P.ex_bpf_base.push_back((int32_t)off_bpf_code[e + 1]);
      P.ex_lvl_base.push_back((int32_t)off_lvl[e + 1]);
      P.ex_pos_base.push_back((int32_t)off_pos_prof[e + 1]);
      P.max_nl = std::max(P.max_nl, O.nl);
      P.max_edges = std::max(P.max_edges, (int)O.ed.size());
      P.max_bpf = std::max(P.max_bpf, (int)O.bpf_code.size());
      P.max_nlev = std::max(P.max_nlev, O.nlev);
      P.max_len = std::max(P.max_len, ds->ex[e].len);
    }
    const double tq1 = tnow();
#define SK_SIZE(f) P.f.resize(off_##f[n]);
    SK_BIG(SK_SIZE)
#undef SK_SIZE
    const double tq2 = tnow();
    {
      std::atomic<int> nx{0};
      auto copy = [&]() {
        for (int e = nx.fetch_add(1); e < n; e = nx.fetch_add(1)) {
          XOut& O = xo[e];
          for (uint32_t& r : O.gra_row) r += (uint32_t)off_xgrow[e];  // example-local -> dataset row
          for (uint32_t& r : O.xf_gra_row) r += (uint32_t)off_xf_row[e];
#define SK_CPY(f) std::copy(O.f.begin(), O.f.end(), P.f.begin() + off_##f[e]);
          SK_BIG(SK_CPY)
#undef SK_CPY
          O = XOut();  // free as we go
        }
      };
      run_pool(nthr, copy);
    }
    if (tstats) fprintf(stderr, "[sk pack] offsets %.1f ms, resize %.1f ms, copy %.1f ms\n", tq1 - tpx, tq2 - tq1, tnow() - tq2);
#undef SK_BIG
    if (tstats) fprintf(stderr, "[sk pack] keys %.1f ms, x-role %.1f ms (%d threads) + append %.1f ms\n",
                        tp1 - tp0, tpx - tp1, nthr, tnow() - tpx);
    if (std::getenv("SK_PACK_STATS")) {  // diagnostic: rows, unstored rows, slots
      long s_rows = 0, s_nost = 0, s_slots = 0, s_nodes = 0, s_st = 0, s_slab = 0, s_gam = 0, s_phi = 0,
           s_reg = 0;
      for (int e = 0; e < n; ++e) {
        s_rows += P.ex_nlxg[e];
        s_nodes += st_nodes[e];
        s_nost += st_nost[e];
        s_slots += st_slots[e];
        // row reads the kernel issues: slab / Gamma / Phi child records, minus
        // the previous row (taken from registers); stored rows
        uint32_t prev = 0xffffu;
        size_t k = (size_t)P.ex_xgch_base[e];
        for (size_t r = (size_t)P.ex_xg_base[e]; r < (size_t)P.ex_xg_base[e] + P.ex_nlxg[e]; ++r) {
          const int ne = P.xgrow[r].a & 0xff;
          for (int t = 0; t < ne; ++t, ++k) {
            const uint32_t c = P.xg_ch[k] & 0xffffu;
            if (c == prev) ++s_reg;
            else if (c & 0x8000u) ++s_gam;
            else if (c & 0x4000u) ++s_phi;
            else ++s_slab;
          }
          prev = P.xgrow[r].b >> 16;
          s_st += prev < 0x4000u;
        }
      }
      fprintf(stderr,
              "[sk pack] gamma schedule: %ld nodes, %ld rows, %ld unstored, %ld slots; stored %ld, reads: "
              "slab %ld gamma %ld phi %ld, from registers %ld\n",
              s_nodes, s_rows, s_nost, s_slots, s_st, s_slab, s_gam, s_phi, s_reg);
      if (P.shared_sums) {  // the same counts of the factored schedule (the one the kernel runs)
        long f_rows = 0, f_ss = 0, f_repl = 0, f_st = 0, f_slab = 0, f_gam = 0, f_phi = 0, f_reg = 0;
        for (int e = 0; e < n; ++e) {
          f_rows += P.ex_nlxf[e];
          f_ss += P.ex_ss_rows[e];
          f_repl += P.ex_ss_repl[e];
          uint32_t prev = 0xffffu;
          size_t k = (size_t)P.ex_xfch_base[e];
          for (size_t r = (size_t)P.ex_xf_base[e]; r < (size_t)P.ex_xf_base[e] + P.ex_nlxf[e]; ++r) {
            const int ne = P.xf_row[r].a & 0xff;
            for (int t = 0; t < ne; ++t, ++k) {
              const uint32_t c = P.xf_ch[k] & 0xffffu;
              if (c == prev) ++f_reg;
              else if (c & 0x8000u) ++f_gam;
              else if (c & 0x4000u) ++f_phi;
              else ++f_slab;
            }
            prev = P.xf_row[r].b >> 16;
            f_st += prev < 0x4000u;
          }
        }
        fprintf(stderr,
                "[sk pack] factored schedule: %ld rows, %ld shared sums for %ld records; stored %ld, reads: "
                "slab %ld gamma %ld phi %ld, from registers %ld\n",
                f_rows, f_ss, f_repl, f_st, f_slab, f_gam, f_phi, f_reg);
      }
    }
  }
  // the x-role arrays are final: the caller may start uploading them while
  // the y-role records are formed (sk_dataset_upload)
  if (after_x) (*after_x)();
  const double tp2 = tnow();
  {
    std::vector<YOut> yo(yjobs.size());
    const int nthr = (int)std::max<size_t>(1, std::min<size_t>({yjobs.size() / 8 + 1, pcap,
                                                                (size_t)std::max(1u, std::thread::hardware_concurrency())}));
    std::atomic<size_t> next{0};
    YOpts yopt;
    yopt.sweep_lanes_greedy = sweep_lanes_greedy;
    // SK_NO_Y_RENUMBER=1: the y nodes in the plain stable order by length (A/B)
    yopt.renumber = !SK_KNOB("SK_NO_Y_RENUMBER");
    yopt.stats = std::getenv("SK_PACK_STATS") != nullptr;
    SweepCost yc_plain, yc_now;
    long y_renum = 0, mg_plain = 0, mg_now = 0, mg_groups = 0;
    auto work = [&]() {
      for (size_t e = next.fetch_add(1); e < yjobs.size(); e = next.fetch_add(1))
        pack_y(P, yopt, yjobs[e], yo[e]);
    };
    run_pool(nthr, work);
    const double ty1 = tnow();
    // appended at prefix-sum offsets, copied on the threads (as the x role)
    const size_t ny = yo.size();
#define SK_YBIG(X) X(ysc) X(ycs) X(ye2) X(yn_a) X(yn_b) X(yn_c) X(yn_p0) X(yrec) X(yn_w) X(yn_nbp) X(yn_P)
#define SK_OFF(f) std::vector<size_t> off_##f(ny + 1, 0);
    SK_YBIG(SK_OFF)
#undef SK_OFF
    for (size_t e = 0; e < ny; ++e) {
      YOut& Y = yo[e];
      if (!Y.err.empty()) {
        err = Y.err;
        return SK_ERR_INVALID;
      }
#define SK_ACC(f) off_##f[e + 1] = off_##f[e] + Y.f.size();
      SK_YBIG(SK_ACC)
#undef SK_ACC
      P.ex_ysc_base.push_back((int32_t)(off_ysc[e] / 64));
      P.ex_ycs_base.push_back((int32_t)off_ycs[e]);
      P.ex_nch.push_back(Y.nch);
      P.max_nch = std::max(P.max_nch, Y.nch);
      yc_plain.read += Y.cost_plain.read, yc_plain.atomic += Y.cost_plain.atomic;
      yc_now.read += Y.cost.read, yc_now.atomic += Y.cost.atomic;
      y_renum += Y.renumbered;
      mg_plain += Y.mg_plain, mg_now += Y.mg_now, mg_groups += Y.mg_groups;
    }
#define SK_SIZE(f) P.f.resize(off_##f[ny]);
    SK_YBIG(SK_SIZE)
#undef SK_SIZE
    // the renumbered records: the same sizes at the same offsets
#define SK_YRBIG(X) X(ysc) X(ye2) X(yn_a) X(yn_b) X(yn_c) X(yn_p0) X(yrec) X(yn_w) X(yn_nbp) X(yn_P)
    P.y_renumbered = yopt.renumber;
    if (P.y_renumbered) {
#define SK_SIZE(f) P.r_##f.resize(off_##f[ny]);
      SK_YRBIG(SK_SIZE)
#undef SK_SIZE
    }
    next = 0;
    auto copy = [&]() {
      for (size_t e = next.fetch_add(1); e < ny; e = next.fetch_add(1)) {
        YOut& Y = yo[e];
#define SK_CPY(f) std::copy(Y.f.begin(), Y.f.end(), P.f.begin() + off_##f[e]);
        SK_YBIG(SK_CPY)
#undef SK_CPY
        if (P.y_renumbered) {
#define SK_CPY(f) std::copy(Y.r.f.begin(), Y.r.f.end(), P.r_##f.begin() + off_##f[e]);
          SK_YRBIG(SK_CPY)
#undef SK_CPY
        }
        Y = YOut();  // free as we go
      }
    };
    run_pool(nthr, copy);
#undef SK_YRBIG
#undef SK_YBIG
    if (tstats) {
      long tch = 0;
      for (int32_t c : P.ex_nch) tch += c;
      fprintf(stderr, "[sk pack] y-role %.1f ms (%d threads) + append %.1f ms; sweep chunks %ld (%.2f per y)\n",
              ty1 - tp2, nthr, tnow() - ty1, tch, P.ex_nch.empty() ? 0.0 : (double)tch / P.ex_nch.size());
    }
    if (yopt.stats) {  // the sweep's and the MATCH gather's bank model, plain order by length and as packed
      long tch = 0;
      for (int32_t c : P.ex_nch) tch += c;
      const double d = (double)std::max(tch, 1l), g = (double)std::max(mg_groups, 1l);
      fprintf(stderr,
              "[sk pack] sweep bank model over %ld chunks: plain order read %.3f atomic %.3f cycles per chunk, "
              "packed read %.3f atomic %.3f (%ld of %zu y renumbered); MATCH gather read cycles per 64-edge "
              "group: plain %.3f packed %.3f\n",
              tch, yc_plain.read / d, yc_plain.atomic / d, yc_now.read / d, yc_now.atomic / d, y_renum, ny,
              mg_plain / g, mg_now / g);
    }
  }
  return SK_OK;
}

}  // namespace sk

extern "C" {

int sk_dataset_upload(sk_context* ctx, sk_dataset* ds) {
  if (!ctx || !ds) return SK_ERR_INVALID;
  if (ds->uploaded) return ds->device == ctx->device ? SK_OK : sk::fail(ctx, SK_ERR_INVALID, "dataset bound to another device");
  SK_HIP(ctx, hipSetDevice(ctx->device));
  if (sk::ds_pal(ds)) {  // a palindrome dataset has its own image (sk::SimpalSet)
    size_t m = 0;
    for (const sk::Example& X : ds->ex) m += X.pal_key.size();
    if (m > (size_t)INT32_MAX) return sk::fail(ctx, SK_ERR_UNSUPPORTED, "palindrome dataset too large");
    try {
      sk::pack_palindromes(ds);
    } catch (const std::bad_alloc&) {
      return sk::fail(ctx, SK_ERR_ALLOC, "palindrome pack");
    }
    const sk_dataset::PalPack& Q = ds->spack;
    SK_HIP(ctx, sk::upload(ds->buf, Q.ex_off, &ds->sdev.ex_off));
    SK_HIP(ctx, sk::upload(ds->buf, Q.key, &ds->sdev.key));
    SK_HIP(ctx, sk::upload(ds->buf, Q.dist, &ds->sdev.dist));
    SK_HIP(ctx, sk::upload(ds->buf, Q.w, &ds->sdev.w));
    ds->spack.key = std::vector<uint64_t>();  // (the device holds them; the host plan reads the offsets)
    ds->spack.dist = std::vector<int32_t>();
    ds->spack.w = std::vector<float>();
    ds->device = ctx->device;
    ds->uploaded = true;
    return SK_OK;
  }
  if (sk::ds_protein(ds)) {  // a protein dataset has its own image (sk::LaProtSet)
    size_t pos = 0;
    for (const sk::Example& X : ds->ex) pos += (size_t)X.len;
    if (pos > (size_t)INT32_MAX) return sk::fail(ctx, SK_ERR_UNSUPPORTED, "protein dataset too large");
    try {
      sk::pack_protein(ds);
    } catch (const std::bad_alloc&) {
      return sk::fail(ctx, SK_ERR_ALLOC, "protein pack");
    }
    const sk_dataset::ProtPack& Q = ds->ppack;
    SK_HIP(ctx, sk::upload(ds->buf, Q.ex_len, &ds->pdev.ex_len));
    SK_HIP(ctx, sk::upload(ds->buf, Q.ex_pos_base, &ds->pdev.ex_pos_base));
    SK_HIP(ctx, sk::upload(ds->buf, Q.prof, &ds->pdev.prof));
    SK_HIP(ctx, sk::upload(ds->buf, Q.code, &ds->pdev.code));
    ds->ppack.prof = std::vector<float>();  // (the device holds them; the host plan reads lengths and flags)
    ds->ppack.code = std::vector<uint8_t>();
    ds->device = ctx->device;
    ds->uploaded = true;
    return SK_OK;
  }
  std::string err;
  sk::HostPack& P = ds->pack;
  sk::DevSet& D = ds->dev;
  sk::DeviceBuffers& B = ds->buf;
  const bool stats = std::getenv("SK_HOST_STATS") != nullptr;
  const auto tu0 = std::chrono::steady_clock::now();
  // the x-role arrays go to the device on a second host thread while the
  // y-role records are formed (pack_dataset calls after_x between the two)
  std::thread xt;
  hipError_t xe = hipSuccess;
  double x_ms = 0.0;
  auto up_x = [&]() -> hipError_t {
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return e;
#define SK_UPX(f, d) \
  if ((e = sk::upload(B, P.f, &D.d)) != hipSuccess) return e;
    SK_UPX(ex_nl, ex_nl)
    SK_UPX(ex_node_base, ex_node_base)
    SK_UPX(ex_edge_base, ex_edge_base)
    SK_UPX(ex_bpf_base, ex_bpf_base)
    SK_UPX(ex_lvl_base, ex_lvl_base)
    SK_UPX(ex_nlev, ex_nlev)
    SK_UPX(ex_nseqs, ex_nseqs)
    SK_UPX(ex_len, ex_len)
    SK_UPX(ex_pos_base, ex_pos_base)
    SK_UPX(ex_has_w, ex_has_w)
    SK_UPX(nd_a, nd_a)
    SK_UPX(nd_b, nd_b)
    SK_UPX(nd_c, nd_c)
    SK_UPX(nd_w, nd_w)
    SK_UPX(nd_nbp, nd_nbp)
    SK_UPX(nd_P, nd_P)
    SK_UPX(ed, ed)
    SK_UPX(bpf_code, bpf_code)
    SK_UPX(bpf_p, bpf_p)
    SK_UPX(lvl, lvl)
    SK_UPX(pos_prof, pos_prof)
    SK_UPX(pos_w, pos_w)
    SK_UPX(pos_chr, pos_chr)
    SK_UPX(pos_lru, pos_lru)
    SK_UPX(ex_nslots, ex_nslots)
    SK_UPX(ex_xch_base, ex_xch_base)
    SK_UPX(xrow, xrow)
    SK_UPX(xr_node, xr_node)
    SK_UPX(xr_ch, xr_ch)
    // the gamma schedule the kernel runs: the factored one where it was built
    if (P.shared_sums) {
      SK_UPX(xf_row, xgrow)
      SK_UPX(xf_node, xg_node)
      SK_UPX(xf_ch, xg_ch)
      SK_UPX(xf_clg, xg_clg)
      SK_UPX(xf_cpf, xg_cpf)
      SK_UPX(xf_cty, xg_cty)
      SK_UPX(xf_gra_row, gra_row)
      SK_UPX(ex_xf_base, ex_xg_base)
      SK_UPX(ex_nlxf, ex_nlxg)
      SK_UPX(ex_xfch_base, ex_xgch_base)
    } else {
      SK_UPX(xgrow, xgrow)
      SK_UPX(xg_node, xg_node)
      SK_UPX(xg_ch, xg_ch)
      SK_UPX(xg_clg, xg_clg)
      SK_UPX(xg_cpf, xg_cpf)
      SK_UPX(xg_cty, xg_cty)
      SK_UPX(gra_row, gra_row)
      SK_UPX(ex_xg_base, ex_xg_base)
      SK_UPX(ex_nlxg, ex_nlxg)
      SK_UPX(ex_xgch_base, ex_xgch_base)
    }
    SK_UPX(gr_info, gr_info)
    SK_UPX(gr_pf, gr_pf)
    SK_UPX(gr_P, gr_P)
    SK_UPX(ex_gapless, ex_gapless)
    SK_UPX(gam_key, gam_key)
    SK_UPX(gra_gidx, gra_gidx)
    SK_UPX(phk_idx, phk_idx)
    SK_UPX(phi_al, phi_al)
    SK_UPX(phi_g, phi_g)
    {
      std::vector<int32_t> grb = P.ex_gr_base;
      grb.push_back((int32_t)P.gr_info.size());
      if ((e = sk::upload(B, grb, &D.ex_gr_base)) != hipSuccess) return e;
      std::vector<int32_t> b1 = P.ex_gra_base, b2 = P.ex_phk_base;
      b1.push_back((int32_t)P.gra_gidx.size());
      b2.push_back((int32_t)P.phk_idx.size());
      if ((e = sk::upload(B, b1, &D.ex_gra_base)) != hipSuccess) return e;
      if ((e = sk::upload(B, b2, &D.ex_phk_base)) != hipSuccess) return e;
    }
#undef SK_UPX
    return hipSuccess;
  };
  const std::function<void()> after_x = [&]() {
    P.xr_ch.insert(P.xr_ch.end(), 8, 0u);  // the kernel prefetches 4 records past a row
    P.xg_ch.insert(P.xg_ch.end(), 8, 0u);
    if (P.shared_sums) P.xf_ch.insert(P.xf_ch.end(), 8, 0u);
    auto job = [&]() {
      const auto t0 = std::chrono::steady_clock::now();
      xe = up_x();
      x_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    try {
      xt = std::thread(job);
    } catch (const std::system_error&) {
      job();  // no second thread: upload them here, before the y-role pack
    }
  };
  int rc = sk::pack_dataset(ds, err, &after_x);
  if (xt.joinable()) xt.join();
  if (rc) return sk::fail(ctx, rc, err);
  SK_HIP(ctx, xe);
  const auto tu1 = std::chrono::steady_clock::now();
  D.n_examples = (int32_t)ds->ex.size();
  // the y records the kernel runs: the renumbered ones where they were formed
  const bool yr = P.y_renumbered;
  SK_HIP(ctx, sk::upload(B, yr ? P.r_yn_a : P.yn_a, &D.yn_a));
  SK_HIP(ctx, sk::upload(B, yr ? P.r_yn_b : P.yn_b, &D.yn_b));
  SK_HIP(ctx, sk::upload(B, yr ? P.r_yn_w : P.yn_w, &D.yn_w));
  SK_HIP(ctx, sk::upload(B, yr ? P.r_yn_nbp : P.yn_nbp, &D.yn_nbp));
  SK_HIP(ctx, sk::upload(B, yr ? P.r_yn_P : P.yn_P, &D.yn_P));
  SK_HIP(ctx, sk::upload(B, yr ? P.r_ysc : P.ysc, &D.ysc));
  SK_HIP(ctx, sk::upload(B, yr ? P.r_ye2 : P.ye2, &D.ye2));
  SK_HIP(ctx, sk::upload(B, yr ? P.r_yn_c : P.yn_c, &D.yn_c));
  SK_HIP(ctx, sk::upload(B, yr ? P.r_yn_p0 : P.yn_p0, &D.yn_p0));
  SK_HIP(ctx, sk::upload(B, P.ycs, &D.ycs));
  SK_HIP(ctx, sk::upload(B, yr ? P.r_yrec : P.yrec, &D.yrec));
  SK_HIP(ctx, sk::upload(B, P.ex_ysc_base, &D.ex_ysc_base));
  SK_HIP(ctx, sk::upload(B, P.ex_nch, &D.ex_nch));
  SK_HIP(ctx, sk::upload(B, P.ex_ycs_base, &D.ex_ycs_base));
  D.n_gam = (int32_t)P.gam_key.size();
  D.n_phi = (int32_t)P.phi_al.size();
  D.max_nl = P.max_nl;
  D.max_edges = P.max_edges;
  D.max_bpf = P.max_bpf;
  D.max_nlev = P.max_nlev;
  D.max_nch = P.max_nch;
  D.max_len = P.max_len;
  D.max_slots = P.max_slots;
  D.total_nodes = (int64_t)P.nd_a.size();
  ds->device = ctx->device;
  ds->uploaded = true;
  if (stats) {
    const auto tu2 = std::chrono::steady_clock::now();
    std::fprintf(stderr,
                 "[sk upload] pack + x-role arrays %.1f ms (x-role transfer %.1f ms beside the y-role pack), %zu arrays "
                 "%.1f MB in all, y-role transfer %.1f ms\n",
                 std::chrono::duration<double, std::milli>(tu1 - tu0).count(), x_ms, B.ptrs.size(), B.bytes / 1e6,
                 std::chrono::duration<double, std::milli>(tu2 - tu1).count());
  }
  return SK_OK;
}

int sk_dataset_sweep_conflicts(const sk_dataset* ds, int i, int32_t* read_cycles, int32_t* atomic_cycles,
                               int32_t* chunks) {
  if (!ds) return SK_ERR_INVALID;
  if (i < 0 || i >= (int)ds->ex.size()) return SK_ERR_RANGE;
  const sk::HostPack& P = ds->pack;
  if (P.ex_nch.size() != ds->ex.size()) return SK_ERR_INVALID;  // not packed yet
  long rd = 0, at = 0;
  for (int c = 0; c < P.ex_nch[i]; ++c) {
    int r1, a1;
    sk::sweep_chunk_cost(P.run_ysc().data() + ((size_t)P.ex_ysc_base[i] + c) * 64, &r1, &a1);
    rd += r1;
    at += a1;
  }
  if (read_cycles) *read_cycles = (int32_t)rd;
  if (atomic_cycles) *atomic_cycles = (int32_t)at;
  if (chunks) *chunks = P.ex_nch[i];
  return SK_OK;
}

int sk_dataset_y_role(const sk_dataset* ds, int i, int plain, int32_t* n_nodes, int32_t* n_edges, int32_t* n_chunks,
                      int32_t* max_len, uint32_t* node, uint32_t* len, uint32_t* edges, uint32_t* sweep,
                      int32_t* first_chunk, int32_t* cost) {
  if (!ds) return SK_ERR_INVALID;
  if (i < 0 || i >= (int)ds->ex.size()) return SK_ERR_RANGE;
  if (sk::ds_pal(ds) || sk::ds_protein(ds)) return SK_ERR_INVALID;
  try {
    // the example packed alone: its x-role node records (no key tables: they
    // do not enter the y role), then its y role in the order asked for
    sk::XOut O;
    sk::pack_x(ds->ex[i], sk::KeyTables(), O);
    if (O.rc) return O.rc;
    sk::HostPack P;
#define SK_MV(f) P.f.assign(O.f.begin(), O.f.end());
    SK_MV(nd_a) SK_MV(nd_b) SK_MV(nd_c) SK_MV(nd_w) SK_MV(nd_nbp) SK_MV(nd_P) SK_MV(ed) SK_MV(bpf_code) SK_MV(bpf_p)
#undef SK_MV
    sk::YOpts opt;
    const char* lanes_env = SK_KNOB("SK_SWEEP_LANES");
    opt.sweep_lanes_greedy = !lanes_env || std::atoi(lanes_env) != 0;
    opt.renumber = !plain && !SK_KNOB("SK_NO_Y_RENUMBER");
    sk::YOut Y;
    sk::pack_y(P, opt, sk::YJob{0, 0, 0, O.nl, O.big}, Y);
    if (!Y.err.empty()) return SK_ERR_INVALID;
    const sk::YRec& R = opt.renumber ? Y.r : Y;
    if (n_nodes) *n_nodes = O.nl;
    if (n_edges) *n_edges = (int32_t)R.ye2.size();
    if (n_chunks) *n_chunks = Y.nch;
    if (max_len) *max_len = (int32_t)Y.ycs.size() - 2;
    if (node) std::copy(R.src.begin(), R.src.end(), node);
    if (len)
      for (int k = 0; k < O.nl; ++k) len[k] = R.yn_b[k] & 0xffff;
    if (edges) std::copy(R.ye2.begin(), R.ye2.end(), edges);
    if (sweep) std::copy(R.ysc.begin(), R.ysc.end(), sweep);
    if (first_chunk) std::copy(Y.ycs.begin(), Y.ycs.end(), first_chunk);
    if (cost) {
      cost[0] = (int32_t)(opt.renumber ? Y.cost : Y.cost_plain).read;
      cost[1] = (int32_t)(opt.renumber ? Y.cost : Y.cost_plain).atomic;
      cost[2] = (int32_t)Y.cost_plain.read;
      cost[3] = (int32_t)Y.cost_plain.atomic;
    }
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
  return SK_OK;
}

int sk_dataset_pack_digest(sk_dataset* ds, uint64_t* y_hash, uint64_t* x_hash) {
  if (!ds || !y_hash || !x_hash) return SK_ERR_INVALID;
  if (ds->uploaded) return SK_ERR_INVALID;
  auto hv = [](const auto& v, uint64_t h) {
    typedef typename std::decay_t<decltype(v)>::value_type T;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h ^ v.size();
  };
  uint64_t hy = 1469598103934665603ull, hx = hy;
  if (sk::ds_pal(ds)) {  // y role: the entries; x role: the runs
    try {
      sk::pack_palindromes(ds);
    } catch (const std::bad_alloc&) {
      return SK_ERR_ALLOC;
    }
    const sk_dataset::PalPack& Q = ds->spack;
    *y_hash = hv(Q.w, hv(Q.dist, hv(Q.key, hy)));
    *x_hash = hv(Q.ex_off, hx);
    ds->spack = sk_dataset::PalPack();
    return SK_OK;
  }
  if (sk::ds_protein(ds)) {  // y role: the columns; x role: the rest
    try {
      sk::pack_protein(ds);
    } catch (const std::bad_alloc&) {
      return SK_ERR_ALLOC;
    }
    const sk_dataset::ProtPack& Q = ds->ppack;
    *y_hash = hv(Q.code, hv(Q.prof, hy));
    *x_hash = hv(Q.ex_coded, hv(Q.ex_pos_base, hv(Q.ex_len, hx)));
    ds->ppack = sk_dataset::ProtPack();
    return SK_OK;
  }
  std::string err;
  const int rc = sk::pack_dataset(ds, err);
  if (rc) return rc;
  const sk::HostPack& P = ds->pack;
#define SK_DG_Y(f) hy = hv(P.f, hy);
#define SK_DG_X(f) hx = hv(P.f, hx);
  SK_PACK_Y_ARRAYS(SK_DG_Y)
  SK_PACK_YR_ARRAYS(SK_DG_Y)
  SK_PACK_X_ARRAYS(SK_DG_X)
#undef SK_DG_Y
#undef SK_DG_X
  *y_hash = hy;
  *x_hash = hx;
  ds->pack = sk::HostPack();  // (the upload packs again: do not hold the arrays until then)
  return SK_OK;
}

}  // extern "C"
