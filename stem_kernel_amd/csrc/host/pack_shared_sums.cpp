// Shared child sums of the gamma schedule.
//
// A child's weight in a row's child sum S_p = sum_c g^gaps(p,c) G0_c factors:
// for a set C of children that two rows read, the two rows' gap exponents on
// C differ by one constant.  So Z_C = sum_{c in C} g^{rel(c)} [g^lg pf] G0_c,
// rel(c) = gaps(p,c) - min_C gaps(p,.), is the same row for every such p, and
// each p reads it with weight g^{min_C gaps(p,.)} in place of the whole set.
// Z_C is a combination row as the kernel runs the phi rows: flag bit 31,
// G0 = S, no MATCH, no sweep, no K term (P = 0).  The test here is on the gap
// exponents themselves, not on the nodes' intervals, so every exponent of
// the factored schedule is at most one of the plain schedule's.
#include "host/pack_shared_sums.h"

#include <algorithm>
#include <utility>

namespace sk {
namespace {

// pairs a row proposes sets with (the nearest following rows that share two
// children with it) and rounds of the search; the third round still finds
// 0.2 % of the records, later ones next to nothing
constexpr int kPairs = 4, kRounds = 3;
constexpr uint32_t kNear = 8;

// a child's identity within one example: its row (>= 0), or -1 - table key
inline int32_t rec_id(const SsRec& r) { return r.row >= 0 ? r.row : -1 - (int32_t)r.key; }

struct Cand {
  uint32_t off, len;    // its members in the id / rel pools (ascending ids)
  uint64_t hash;
  uint32_t uoff, ulen;  // its users in the user pool
  long value;
};

}  // namespace

bool shared_sums_schedule(std::vector<SsRow>&& in, int threshold, bool store_all, SsOut& out) {
  const int n = (int)in.size();
  std::vector<SsRow> R(std::move(in));
  out = SsOut();
  int32_t nkeys = 0;  // table keys are below this
  for (const SsRow& W : R)
    if (W.user)
      for (const SsRec& r : W.rec)
        if (r.row < 0) nkeys = std::max(nkeys, (int32_t)r.key + 1);

  // ---- the search: rounds of pairwise intersections, applied best first.
  // All lists are flat (offsets into pools): the pass runs per example of a
  // dataset and must stay a fraction of the packer's time.
  typedef std::pair<int32_t, uint32_t> Mem;  // (id, gaps)
  std::vector<Mem> mem, tmp, mem_prev;
  std::vector<uint32_t> moff(n + 1), moff_prev, poff, pfill;
  std::vector<int32_t> par, idpool, upool;
  std::vector<uint32_t> relpool;
  std::vector<Cand> cands;
  std::vector<uint32_t> keep;
  std::vector<int> cnt(n, 0), seen, us;
  std::vector<std::pair<int64_t, uint32_t>> com;
  std::vector<uint8_t> touched(n);
  for (int round = 0; round < kRounds; ++round) {
    // every user's members: the type 0 / 1 records whose child the row reads
    // once (a child read twice stays as plain records), ascending ids
    // (a row the last round left alone keeps its list)
    mem.swap(mem_prev);
    moff.swap(moff_prev);
    moff.resize(n + 1);
    mem.clear();
    for (int u = 0; u < n; ++u) {
      moff[u] = (uint32_t)mem.size();
      if (!R[u].user) continue;
      if (round > 0 && !touched[u]) {
        mem.insert(mem.end(), mem_prev.begin() + moff_prev[u], mem_prev.begin() + moff_prev[u + 1]);
        continue;
      }
      tmp.clear();
      for (const SsRec& r : R[u].rec)
        if (r.cty <= 1) tmp.push_back({rec_id(r), r.gaps});
      std::sort(tmp.begin(), tmp.end());
      for (size_t i = 0; i < tmp.size();) {
        size_t j = i + 1;
        while (j < tmp.size() && tmp[j].first == tmp[i].first) ++j;
        if (j == i + 1) mem.push_back(tmp[i]);
        i = j;
      }
    }
    moff[n] = (uint32_t)mem.size();
    // child -> its users, ascending (CSR over rows, then table keys)
    const int32_t nrow = (int32_t)R.size();
    auto slot_of = [&](int32_t id) { return id >= 0 ? id : nrow + (-1 - id); };
    poff.assign((size_t)nrow + nkeys + 1, 0u);
    for (const Mem& m : mem) ++poff[slot_of(m.first) + 1];
    for (size_t i = 0; i + 1 < poff.size(); ++i) poff[i + 1] += poff[i];
    pfill.assign(poff.begin(), poff.end() - 1);
    par.resize(mem.size());
    for (int u = 0; u < n; ++u)
      for (uint32_t i = moff[u]; i < moff[u + 1]; ++i) par[pfill[slot_of(mem[i].first)]++] = u;
    pfill.assign(poff.begin(), poff.end() - 1);
    // candidate sets
    cands.clear();
    idpool.clear();
    relpool.clear();
    for (int u = 0; u < n; ++u) {
      const Mem* mu = mem.data() + moff[u];
      const uint32_t nu = moff[u + 1] - moff[u];
      if (nu < 2) continue;
      // the rows after u that share children with it: of each child's
      // users the next kNear (pfill: the first one after u; u ascends)
      seen.clear();
      for (uint32_t i = 0; i < nu; ++i) {
        const int32_t sl = slot_of(mu[i].first);
        uint32_t& cur = pfill[sl];
        while (cur < poff[sl + 1] && par[cur] <= u) ++cur;
        for (uint32_t t = cur; t < poff[sl + 1] && t < cur + kNear; ++t)
          if (cnt[par[t]]++ == 0) seen.push_back(par[t]);
      }
      std::sort(seen.begin(), seen.end());
      int npair = 0;
      for (int v : seen) {
        const int c = cnt[v];
        cnt[v] = 0;
        // (a set's users are found from the children's parent lists below,
        // whichever pair proposed it)
        if (c < 2 || npair >= kPairs) continue;
        // (a pair the last round left alone proposed its set then)
        if (round > 0 && !touched[u] && !touched[v]) continue;
        ++npair;
        // common children by gap difference; the most frequent difference
        const Mem* mv = mem.data() + moff[v];
        const uint32_t nv = moff[v + 1] - moff[v];
        com.clear();
        for (uint32_t i = 0, j = 0; i < nu && j < nv;) {
          if (mu[i].first < mv[j].first) ++i;
          else if (mv[j].first < mu[i].first) ++j;
          else {
            com.push_back({(int64_t)mu[i].second - (int64_t)mv[j].second, i});
            ++i, ++j;
          }
        }
        std::sort(com.begin(), com.end());
        size_t b0 = 0, bl = 0;
        for (size_t i = 0; i < com.size();) {
          size_t j = i + 1;
          while (j < com.size() && com[j].first == com[i].first) ++j;
          if (j - i > bl) bl = j - i, b0 = i;
          i = j;
        }
        if (bl < 2) continue;
        Cand cd{(uint32_t)idpool.size(), (uint32_t)bl, 1469598103934665603ull, 0u, 0u, 0};
        uint32_t mn = 0xffffffffu;
        for (size_t i = b0; i < b0 + bl; ++i) mn = std::min(mn, mu[com[i].second].second);
        for (size_t i = b0; i < b0 + bl; ++i) {  // (ascending index = ascending id)
          idpool.push_back(mu[com[i].second].first);
          relpool.push_back(mu[com[i].second].second - mn);
          cd.hash = (cd.hash ^ (uint32_t)idpool.back()) * 1099511628211ull;
        }
        cands.push_back(cd);
      }
    }
    keep.resize(cands.size());
    for (size_t i = 0; i < cands.size(); ++i) keep[i] = (uint32_t)i;
    auto same = [&](const Cand& a, const Cand& b) {
      return a.hash == b.hash && a.len == b.len &&
             std::equal(idpool.begin() + a.off, idpool.begin() + a.off + a.len, idpool.begin() + b.off);
    };
    std::sort(keep.begin(), keep.end(), [&](uint32_t a, uint32_t b) {
      return cands[a].hash != cands[b].hash ? cands[a].hash < cands[b].hash : a < b;
    });
    {
      size_t o = 0;
      for (size_t i = 0; i < keep.size(); ++i) {
        bool dup = false;
        for (size_t j = o; j-- > 0 && cands[keep[j]].hash == cands[keep[i]].hash && !dup;)
          dup = same(cands[keep[j]], cands[keep[i]]);
        if (!dup) keep[o++] = keep[i];
      }
      keep.resize(o);
    }
    std::sort(keep.begin(), keep.end());
    // every set's users: the rows holding all its members at the same
    // relative exponents
    upool.clear();
    {
      size_t o = 0;
      for (uint32_t ci : keep) {
        Cand& cd = cands[ci];
        const int32_t* ids = idpool.data() + cd.off;
        const uint32_t* rel = relpool.data() + cd.off;
        int32_t least = slot_of(ids[0]);
        for (uint32_t t = 1; t < cd.len; ++t) {
          const int32_t sl = slot_of(ids[t]);
          if (poff[sl + 1] - poff[sl] < poff[least + 1] - poff[least]) least = sl;
        }
        cd.uoff = (uint32_t)upool.size();
        for (uint32_t q = poff[least]; q < poff[least + 1]; ++q) {
          const int u = par[q];
          const Mem* mu = mem.data() + moff[u];
          const uint32_t nu = moff[u + 1] - moff[u];
          uint32_t i = 0;
          int64_t d = 0;
          bool ok = true;
          for (uint32_t t = 0; t < cd.len && ok; ++t) {
            while (i < nu && mu[i].first < ids[t]) ++i;
            ok = i < nu && mu[i].first == ids[t] && mu[i].second >= rel[t];
            if (!ok) break;
            const int64_t dt = (int64_t)mu[i].second - rel[t];
            if (t == 0) d = dt;
            ok = dt == d;
          }
          if (ok) upool.push_back(u);
        }
        cd.ulen = (uint32_t)upool.size() - cd.uoff;
        const long k = (long)cd.ulen, s = (long)cd.len;
        cd.value = k * s - (s + 1 + k) - threshold;
        if (k >= 2 && cd.value > 0) keep[o++] = ci;
      }
      keep.resize(o);
    }
    std::stable_sort(keep.begin(), keep.end(), [&](uint32_t a, uint32_t b) { return cands[a].value > cands[b].value; });
    std::fill(touched.begin(), touched.end(), 0);
    int applied = 0;
    for (uint32_t ci : keep) {
      const Cand& cd = cands[ci];
      const int32_t* ids = idpool.data() + cd.off;
      us.clear();
      for (uint32_t q = 0; q < cd.ulen; ++q)
        if (!touched[upool[cd.uoff + q]]) us.push_back(upool[cd.uoff + q]);
      const long k = (long)us.size(), s = (long)cd.len;
      if (k < 2 || k * s - (s + 1 + k) - threshold <= 0) continue;
      const int z = (int)R.size();
      SsRow Z;
      Z.xr = XRow{0u, 0u, 0x80000000u, 0.0f, 0.0f, 0.0f, 0.0};
      Z.node = R[us[0]].node;
      Z.user = false;
      Z.swept = false;
      for (uint32_t t = 0; t < cd.len; ++t)
        for (const SsRec& r : R[us[0]].rec)
          if (r.cty <= 1 && rec_id(r) == ids[t]) {
            SsRec m = r;
            m.gaps = relpool[cd.off + t];
            Z.rec.push_back(m);
          }
      for (int u : us) {
        std::vector<SsRec> nr;
        nr.reserve(R[u].rec.size());
        uint32_t mg = 0xffffffffu;
        size_t at = R[u].rec.size();
        for (const SsRec& r : R[u].rec) {
          if (r.cty <= 1 && std::binary_search(ids, ids + cd.len, rec_id(r))) {
            mg = std::min(mg, r.gaps);
            at = std::min(at, nr.size());
          } else {
            nr.push_back(r);
          }
        }
        // the shared sum's record, among the row's first four
        const SsRec zr{z, 0u, 0u, mg, 0u, 1.0f, 0};
        nr.insert(nr.begin() + std::min<size_t>(at, 3), zr);
        R[u].rec.swap(nr);
        touched[u] = 1;
        out.n_replaced += (int)s;
      }
      R.push_back(std::move(Z));
      ++out.n_shared;
      ++applied;
    }
    if (!applied) break;
  }

  // ---- the order: the input rows as they were; a shared-sum row directly
  // after its last member row (it takes that member from registers), one
  // whose members are all table rows directly before its first user
  const int nr = (int)R.size();
  std::vector<int> gap(nr, -1);  // shared-sum row: placed after input row gap[z] (-1: at the front)
  std::vector<int> ready(nr, -1);
  for (int r = 0; r < n; ++r) ready[r] = r;
  for (int z = n; z < nr; ++z)
    for (const SsRec& m : R[z].rec)
      if (m.row >= 0) ready[z] = std::max(ready[z], ready[m.row]);
  {
    std::vector<int> need(nr, n);
    for (int r = 0; r < n; ++r)
      for (const SsRec& m : R[r].rec)
        if (m.row >= n) need[m.row] = std::min(need[m.row], r - 1);
    for (int z = nr - 1; z >= n; --z) {  // users were made after their members
      gap[z] = ready[z] >= 0 ? ready[z] : need[z];
      for (const SsRec& m : R[z].rec)
        if (m.row >= n) need[m.row] = std::min(need[m.row], gap[z]);
    }
  }
  std::vector<int> order;
  order.reserve(nr);
  {
    std::vector<int> goff(n + 2, 0), gl(nr - n);
    for (int z = n; z < nr; ++z) ++goff[gap[z] + 2];
    for (int i = 0; i <= n; ++i) goff[i + 1] += goff[i];
    std::vector<int> gf(goff.begin(), goff.end() - 1);
    for (int z = n; z < nr; ++z) gl[gf[gap[z] + 1]++] = z;  // creation order within a gap
    for (int g = -1; g < n; ++g) {
      if (g >= 0) order.push_back(g);
      for (int i = goff[g + 1]; i < goff[g + 2]; ++i) order.push_back(gl[i]);
    }
  }
  std::vector<int> pos(nr, -1);
  for (int i = 0; i < nr; ++i) pos[order[i]] = i;
  // a shared-sum row's record of the row before it goes first
  for (int i = 1; i < nr; ++i) {
    const int z = order[i];
    if (z < n) continue;
    std::vector<SsRec>& rec = R[z].rec;
    for (size_t t = 0; t < rec.size(); ++t)
      if (rec[t].row == order[i - 1]) {
        std::rotate(rec.begin(), rec.begin() + t, rec.begin() + t + 1);
        break;
      }
  }
  // every child row before its reader
  for (int r = 0; r < nr; ++r) {
    if (R[r].rec.size() > 255) return false;
    for (const SsRec& m : R[r].rec)
      if (m.row >= 0 && pos[m.row] >= pos[r]) return false;
  }

  // ---- slots, by the plain schedule's rules on this order: a row's slot is
  // freed at its last reader (LIFO); a row read once, by the next row among
  // its first four records, is never stored (0xfffe); a row nobody reads has
  // no slot (0xffff)
  std::vector<int> npar(nr, 0), last(nr, -1);
  for (int i = 0; i < nr; ++i)
    for (const SsRec& m : R[order[i]].rec)
      if (m.row >= 0) {
        ++npar[m.row];
        last[m.row] = order[i];
      }
  std::vector<uint8_t> nostore(nr, 0);
  for (int i = 0; i + 1 < nr && !store_all; ++i) {
    const int v = order[i], r = order[i + 1];
    if (npar[v] != 1 || !(R[r].swept || r >= n)) continue;
    for (size_t t = 0; t < R[r].rec.size() && t < 4; ++t)
      if (R[r].rec[t].row == v) nostore[v] = 1;
  }
  std::vector<uint32_t> slot(nr, 0xffffu);
  std::vector<int> freel;
  int nslots = 0;
  out.new_index.assign(n, 0u);
  out.row.reserve(nr);
  out.node.reserve(nr);
  {
    size_t nrec = 0;
    for (const SsRow& W : R) nrec += W.rec.size();
    out.ch.reserve(nrec);
    out.clg.reserve(nrec);
    out.cpf.reserve(nrec);
    out.cty.reserve(nrec);
  }
  for (int i = 0; i < nr; ++i) {
    const int v = order[i];
    const SsRow& W = R[v];
    for (const SsRec& m : W.rec) {
      out.ch.push_back((m.row >= 0 ? (slot[m.row] & 0xffffu) : m.lo) | (m.gaps << 16));
      out.clg.push_back(m.clg);
      out.cpf.push_back(m.cpf);
      out.cty.push_back(m.cty);
      if (m.gaps > 0xffffu) return false;
    }
    for (const SsRec& m : W.rec)
      if (m.row >= 0 && last[m.row] == v && slot[m.row] < 0x4000u) {
        freel.push_back((int)slot[m.row]);
        slot[m.row] |= 0x10000u;  // freed (a second record of the child must not free it again)
      }
    if (nostore[v]) {
      slot[v] = 0xfffeu;
    } else if (npar[v] > 0) {
      if (!freel.empty()) {
        slot[v] = (uint32_t)freel.back();
        freel.pop_back();
      } else {
        slot[v] = (uint32_t)nslots++;
      }
    }
    XRow xr = W.xr;
    xr.a = (xr.a & ~0xffu) | (uint32_t)W.rec.size();
    xr.b = (xr.b & 0xffffu) | (slot[v] << 16);
    out.row.push_back(xr);
    out.node.push_back(W.node);
    if (v < n) out.new_index[v] = (uint32_t)i;
  }
  out.nslots = nslots;
  return nslots < 0x4000;
}

}  // namespace sk
