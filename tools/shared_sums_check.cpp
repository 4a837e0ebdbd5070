// Schedule equivalence check of the factored gamma schedule (CPU only): packs
// a synthetic dataset with the library's sk::pack_dataset and, per example,
// runs both gamma schedules symbolically -- the plain one (xg_*) and the
// factored one (xf_*, host/pack_shared_sums.cpp) -- resolving every child
// record to the row that last wrote its slot.  It checks that
//   - every real row of the factored schedule, its shared-sum records
//     expanded recursively, reads exactly the plain row's multiset of
//     (child, total gap exponent, lg, pf, type); a slot reassigned while a
//     reader was pending would resolve to another child and fail here;
//   - every child row was produced before it is read, a never-stored row
//     (slot 0xfffe) is read once, by the next row among its first four
//     records, and a row without a slot (0xffff) is never read;
//   - the limits of the layout hold: at most 255 records per row, slots below
//     0x4000 and max_slots, exponents inside the gap-power table;
//   - shared-sum rows are combination rows with P = 0 outside gra_row, and the
//     real rows keep their records' other fields;
//   - the dataset has shared-sum rows at all.
// Prints "ok shared=<rows> replaced=<records> f-hash <hash of the xf arrays>"
// and exits 0, or the first failure and exits 1.  Build like pack_compare.cpp.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "host/runtime_types.h"

using sk::HostPack;
template <class V> static uint64_t hv(const V& v, uint64_t h) {
  typedef typename V::value_type T;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h ^ v.size();
}

// (kind: 0 real row by ordinal, 1 table row; id; gap; lg; pf bits; type)
typedef std::tuple<int, uint32_t, uint32_t, uint32_t, uint32_t, int> Term;

static int fail(int e, size_t r, const char* what) {
  printf("FAIL example %d row %zu: %s\n", e, r, what);
  return 1;
}

struct Sched {
  const sk::XRow* row;
  const uint32_t *ch, *clg;
  const float* cpf;
  const uint8_t* cty;
  int n;
};

// the rows' expansions, in schedule order; real[r] = ordinal of a real row, -1
// of a shared-sum row
static int expand(int e, const Sched& S, int max_slots, uint32_t max_gap, std::vector<std::vector<Term>>& out,
                  std::vector<int>& real) {
  std::vector<int> occ((size_t)max_slots, -1), nread(S.n, 0);
  std::vector<std::vector<Term>> ex(S.n);
  real.assign(S.n, -1);
  int nreal = 0;
  size_t k = 0;
  for (int r = 0; r < S.n; ++r) {
    const sk::XRow& xr = S.row[r];
    const int ne = xr.a & 0xff;
    const bool combo = (xr.c >> 31) != 0u;
    const bool shared = combo && ne > 0 && S.cty[k] <= 1;
    if (shared) {
      if (xr.P != 0.0) return fail(e, r, "a shared-sum row with P != 0");
      if (ne < 2) return fail(e, r, "a shared-sum row with fewer than two members");
    } else {
      real[r] = nreal++;
    }
    for (int t = 0; t < ne; ++t, ++k) {
      const uint32_t c = S.ch[k] & 0xffffu, g = S.ch[k] >> 16;
      uint32_t pfb;
      std::memcpy(&pfb, &S.cpf[k], 4);
      if (g > max_gap || S.clg[k] > max_gap) return fail(e, r, "a gap exponent outside the power table");
      if (shared && S.cty[k] > 1) return fail(e, r, "a shared-sum row with a recipe record");
      if (S.cty[k] != 0) {  // a table row (gamma child, phi component)
        if (!(c & 0xc000u)) return fail(e, r, "a table record without a table flag");
        ex[r].push_back(Term(1, c, g, S.clg[k], pfb, S.cty[k]));
        continue;
      }
      int p;
      if (c == 0xfffeu) {
        p = r - 1;
        if (p < 0 || (S.row[p].b >> 16) != 0xfffeu) return fail(e, r, "a register record whose previous row is stored");
        if (t >= 4) return fail(e, r, "a register record past the fourth");
      } else {
        if (c >= 0x4000u || (int)c >= max_slots) return fail(e, r, "a slot over the limit");
        p = occ[c];
        if (p < 0) return fail(e, r, "a child read before it is produced");
      }
      ++nread[p];
      if (real[p] >= 0) {
        ex[r].push_back(Term(0, (uint32_t)real[p], g, S.clg[k], pfb, 0));
      } else {
        for (const Term& m : ex[p])
          ex[r].push_back(Term(std::get<0>(m), std::get<1>(m), std::get<2>(m) + g, std::get<3>(m), std::get<4>(m),
                               std::get<5>(m)));
      }
    }
    const uint32_t slot = xr.b >> 16;
    if (slot < 0x4000u) {
      if ((int)slot >= max_slots) return fail(e, r, "a slot past max_slots");
      occ[slot] = r;
    } else if (slot != 0xfffeu && slot != 0xffffu) {
      return fail(e, r, "a slot over the limit");
    }
  }
  for (int r = 0; r < S.n; ++r) {
    const uint32_t slot = S.row[r].b >> 16;
    if (slot == 0xffffu && nread[r]) return fail(e, r, "a row without a slot is read");
    if (slot == 0xfffeu && nread[r] != 1) return fail(e, r, "a never-stored row is not read exactly once");
    if (slot < 0x4000u && !nread[r]) return fail(e, r, "a stored row nobody reads");
  }
  out.clear();
  for (int r = 0; r < S.n; ++r)
    if (real[r] >= 0) {
      std::sort(ex[r].begin(), ex[r].end());
      out.push_back(std::move(ex[r]));
    }
  return 0;
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 7;
  const int L = argc > 2 ? atoi(argv[2]) : 40;
  sk_dataset* ds = nullptr;
  sk_dataset_create(&ds);
  uint64_t st = 0x5EED0001ull;
  std::vector<char> buf((size_t)n * (L + 1));
  sk_random_sequences(&st, n, L, buf.data());
  std::vector<std::string> ss(n);
  std::vector<const char*> sp(n);
  for (int i = 0; i < n; ++i) {
    ss[i].assign(&buf[(size_t)i * (L + 1)], L);
    sp[i] = ss[i].c_str();
  }
  int rc = sk_dataset_add_synthetic(ds, n, sp.data(), nullptr, 0.01f, 8);
  std::string err;
  rc |= sk::pack_dataset(ds, err);
  if (rc) {
    printf("FAIL pack rc=%d %s\n", rc, err.c_str());
    return 1;
  }
  const HostPack& P = ds->pack;
  if (!P.shared_sums) {
    printf("FAIL the dataset has no factored schedule\n");
    return 1;
  }
  const uint32_t max_gap = (uint32_t)P.max_len + 1;  // the gap-power table has max_len + 2 entries
  long shared = 0, repl = 0, t_plain = 0, t_fact = 0;
  for (int e = 0; e < n; ++e) {
    const size_t gb = (size_t)P.ex_xg_base[e], gc = (size_t)P.ex_xgch_base[e];
    const size_t fb = (size_t)P.ex_xf_base[e], fc = (size_t)P.ex_xfch_base[e];
    const Sched A{P.xgrow.data() + gb, P.xg_ch.data() + gc, P.xg_clg.data() + gc, P.xg_cpf.data() + gc,
                  P.xg_cty.data() + gc, P.ex_nlxg[e]};
    const Sched B{P.xf_row.data() + fb, P.xf_ch.data() + fc, P.xf_clg.data() + fc, P.xf_cpf.data() + fc,
                  P.xf_cty.data() + fc, P.ex_nlxf[e]};
    std::vector<std::vector<Term>> ea, eb;
    std::vector<int> ra, rb;
    if (expand(e, A, P.max_slots, max_gap, ea, ra) || expand(e, B, P.max_slots, max_gap, eb, rb)) return 1;
    if (ea.size() != eb.size() || (int)ea.size() != A.n) return fail(e, 0, "the schedules' real rows differ in number");
    for (size_t r = 0; r < ea.size(); ++r)
      if (ea[r] != eb[r]) return fail(e, r, "a row's expanded child records differ from the plain schedule's");
    // the real rows' records, in order, but for the child count and the slot
    std::vector<size_t> fidx;
    for (int r = 0; r < B.n; ++r)
      if (rb[r] >= 0) fidx.push_back((size_t)r);
    for (int r = 0; r < A.n; ++r) {
      sk::XRow x = A.row[r], y = B.row[fidx[r]];
      x.a &= ~0xffu, y.a &= ~0xffu, x.b &= 0xffffu, y.b &= 0xffffu;
      if (std::memcmp(&x, &y, sizeof(x)) != 0) return fail(e, (size_t)r, "a real row's record differs");
      if (P.xg_node[gb + r] != P.xf_node[fb + fidx[r]]) return fail(e, (size_t)r, "a real row's node differs");
    }
    for (int r = 0; r < B.n; ++r)
      if (P.xf_node[fb + r] >= (uint32_t)P.ex_nl[e]) return fail(e, (size_t)r, "a row's node is out of range");
    // gra_row names the same phi rows
    const size_t g0 = (size_t)P.ex_gra_base[e], g1 = e + 1 < n ? (size_t)P.ex_gra_base[e + 1] : P.gra_gidx.size();
    for (size_t i = g0; i < g1; ++i) {
      const size_t pr = P.gra_row[i] - gb, fr = P.xf_gra_row[i] - fb;
      if (pr >= (size_t)A.n || fr >= (size_t)B.n || rb[fr] != (int)pr) return fail(e, i, "gra_row names another row");
    }
    int nsh = 0;
    for (int r = 0; r < B.n; ++r) nsh += rb[r] < 0;
    if (nsh != P.ex_ss_rows[e]) return fail(e, 0, "ex_ss_rows miscounts the shared-sum rows");
    shared += nsh;
    repl += P.ex_ss_repl[e];
    for (int r = 0; r < A.n; ++r) t_plain += (A.row[r].a & 0xff) + ((A.row[r].b >> 16) < 0x4000u);
    for (int r = 0; r < B.n; ++r) t_fact += (B.row[r].a & 0xff) + ((B.row[r].b >> 16) < 0x4000u);
  }
  if (!shared) {
    printf("FAIL no shared-sum rows in the set\n");
    return 1;
  }
  uint64_t h = 1469598103934665603ull;
#define SC_H(f) h = hv(P.f, h);
  SK_PACK_F_ARRAYS(SC_H)
  printf("ok n=%d L=%d shared=%ld replaced=%ld records+stores plain=%ld factored=%ld f-hash %016llx\n", n, L, shared,
         repl, t_plain, t_fact, (unsigned long long)h);
  return 0;
}
