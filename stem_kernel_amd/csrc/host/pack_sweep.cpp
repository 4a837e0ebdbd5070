// The LDS bank model of the DAG stem kernel's IY sweep and the packer passes
// that place records through it: the lane dealing of a sweep chunk, the
// renumbering of equal-length y nodes, and the MATCH gather's read model
// (pack_y and sk_dataset_sweep_conflicts call them, host/pack_internal.h).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "host/pack_internal.h"

namespace sk {
namespace {

// LDS bank model of one IY sweep chunk (64 records child:11 | parent:11 |
// gaps:10 in lane order).  The kernel reads R[child] (ds_read_b64: banks by
// element mod 32 within each 32-lane half, one cycle per distinct address of
// the fullest bank) and adds into R[parent] (ds_add_f64: taken as 16-lane
// groups, element mod 16, one cycle per record of the fullest bank, same
// address or not).  The lane dealing below and the renumbering pass both
// place records through it, and sk_dataset_sweep_conflicts reports it.
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

// Lane placement of one IY sweep chunk (records child:11 | parent:11 |
// gaps:10, sorted ids): the edges are dealt to the four 16-lane groups
// greedily to spread the child reads and the parent atomics over the banks
// of SweepBanks, the parents with most edges in the chunk first; dummies
// (child == parent, weight 0) take the emptiest slots.
void assign_sweep_lanes(const int* take, int n, const std::vector<uint32_t>& er, int nl, uint32_t lanes[64]) {
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

}  // namespace

void sweep_chunk_cost(const uint32_t lanes[64], int* read_cycles, int* atomic_cycles) {
  SweepBanks B;
  for (int l = 0; l < 64; ++l) B.put(l >> 4, lanes[l] & 0x7ff, (lanes[l] >> 11) & 0x7ff);
  *read_cycles = B.read_cycles();
  *atomic_cycles = B.atomic_cycles();
}

void sweep_chunk_lanes(const int* take, int n, const std::vector<uint32_t>& er, int nl, bool greedy,
                       uint32_t lanes[64]) {
  if (greedy) return assign_sweep_lanes(take, n, er, nl, lanes);
  for (int j = 0; j < n; ++j) lanes[j] = er[take[j]];
  for (int j = n; j < 64; ++j) {
    const uint32_t d = (uint32_t)(j % std::max(nl, 1));
    lanes[j] = d | (d << 11);
  }
}

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
namespace {
struct Renumbering {
  const SweepSchedule& S;
  std::vector<int>& newid;  // node -> id
  const int nl, nch;
  std::vector<int> who;           // id -> node (-1: free)
  std::vector<int> r0, r1;        // runs of equal length: r0[i] .. r1[i] holds i
  std::vector<int> cread, catom;  // the dealt chunks' cycles
  // a node's chunks: as a child (each chunk once: one address however many
  // lanes read it) and as a parent (with its records there), CSR by node;
  // a parent's edges (contiguous)
  std::vector<int> coff, poff, cinc, pinc, pmul, pfirst, pcount;
  std::vector<uint16_t> rc, ac;  // placed same-bank children (distinct) and parent records per chunk
  std::vector<uint32_t> er;      // S.er in the numbering newid

  Renumbering(const SweepSchedule& S_, std::vector<int>& newid_)
      : S(S_), newid(newid_), nl(S_.nl), nch(S_.nch()), cread(nch), catom(nch) {}

  void deal_cost(int ch, const std::vector<uint32_t>& recs, int* rd, int* at) const {
    uint32_t lanes[64];
    sweep_chunk_lanes(S.chunk_ed.data() + S.chunk_off[ch], S.chunk_off[ch + 1] - S.chunk_off[ch], recs, nl,
                      S.lanes_greedy, lanes);
    sweep_chunk_cost(lanes, rd, at);
  }
  SweepCost deal_all(const std::vector<uint32_t>& recs) {  // (into cread / catom)
    SweepCost c;
    for (int ch = 0; ch < nch; ++ch) {
      deal_cost(ch, recs, &cread[ch], &catom[ch]);
      c.read += cread[ch];
      c.atomic += catom[ch];
    }
    return c;
  }
  bool find_runs(const std::vector<int>& len) {  // false: every run is one node
    r0.resize(nl);
    r1.resize(nl);
    bool any_run = false;
    for (int i = 0; i < nl;) {
      int j = i;
      while (j < nl && len[j] == len[i]) ++j;
      for (int t = i; t < j; ++t) r0[t] = i, r1[t] = j;
      any_run |= j - i > 1;
      i = j;
    }
    return any_run;
  }
  void node_chunks() {
    const int ne = (int)S.er.size();
    coff.assign(nl + 1, 0);
    poff.assign(nl + 1, 0);
    pfirst.assign(nl, -1);
    pcount.assign(nl, 0);
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
    for (int f = ne - 1; f >= 0; --f) pfirst[S.epar[f]] = f, ++pcount[S.epar[f]];
    rc.assign((size_t)nch * 32, 0);
    ac.assign((size_t)nch * 16, 0);
  }
  int score(int v, int id) const {
    int s = 0;
    for (int t = coff[v]; t < coff[v + 1]; ++t) s += rc[(size_t)cinc[t] * 32 + (id & 31)];
    for (int t = poff[v]; t < poff[v + 1]; ++t) s += pmul[t] * ac[(size_t)pinc[t] * 16 + (id & 15)];
    return s;
  }
  void place(int v, int id, int sign) {
    for (int t = coff[v]; t < coff[v + 1]; ++t) rc[(size_t)cinc[t] * 32 + (id & 31)] += sign;
    for (int t = poff[v]; t < poff[v + 1]; ++t) ac[(size_t)pinc[t] * 16 + (id & 15)] += sign * pmul[t];
  }
  void set_id(int v, int id) {  // (in er)
    for (int t = S.cb[v]; t < S.cb[v + 1]; ++t) er[S.by_child[t]] = (er[S.by_child[t]] & ~0x7ffu) | (uint32_t)id;
    for (int f = pfirst[v]; f >= 0 && f < pfirst[v] + pcount[v]; ++f)
      er[f] = (er[f] & ~(0x7ffu << 11)) | ((uint32_t)id << 11);
  }
  // greedy pass: the nodes alone in their run are where they are; the rest
  // by incidence (edges as a child and as a parent), most first, then by id
  void greedy() {
    who.assign(nl, -1);
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
  // the best exchange of ids, by the placed counts, for a node on chunk ch's
  // fullest child or parent bank: node a takes id j (false: none lowers them)
  bool propose_swap(int ch, int it, std::vector<int>& asked, int* a_out, int* j_out) {
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
    *a_out = ba;
    *j_out = bj;
    return ba >= 0;
  }
  // swaps within runs, at most kSwapTries proposals, each for the costliest
  // chunk not given up; kept when the dealt chunks' cost falls (now follows)
  void swaps(SweepCost& now) {
    const int kSwapTries = std::min(nch, 32);
    std::vector<uint8_t> tried(nch, 0);
    std::vector<int> aff, stamp(nch, -1), asked(nl, -1);
    for (int it = 0; it < kSwapTries; ++it) {
      int ch = -1;
      for (int k = 0; k < nch; ++k)
        if (!tried[k] && cread[k] + catom[k] > 6 && (ch < 0 || cread[k] + catom[k] > cread[ch] + catom[ch])) ch = k;
      if (ch < 0) break;
      int ba, bj;
      if (!propose_swap(ch, it, asked, &ba, &bj)) {
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
};
}  // namespace

void renumber_equal_lengths(const SweepSchedule& S, const std::vector<int>& len, std::vector<int>& newid,
                            SweepCost& plain, SweepCost& now) {
  newid.resize(S.nl);
  std::iota(newid.begin(), newid.end(), 0);
  Renumbering R(S, newid);
  plain = now = R.deal_all(S.er);
  if (!R.find_runs(len) || R.nch == 0) return;
  R.node_chunks();
  R.greedy();
  // the dealt cost of that numbering
  R.er = S.er;
  for (int v = 0; v < S.nl; ++v)
    if (newid[v] != v) R.set_id(v, newid[v]);
  now = R.deal_all(R.er);
  R.swaps(now);
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
void match_gather_cost(const std::vector<uint32_t>& child, const std::vector<int>& starts, long* cycles,
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

}  // namespace sk
