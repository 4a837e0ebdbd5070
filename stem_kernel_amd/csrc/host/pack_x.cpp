// The x role of one example (pack_x, host/pack_internal.h) and the dataset's
// key tables.  pack_x runs in phases, each a function below: the node levels,
// the row flags, the path weights, the level-order records, the full x
// schedule, the gamma schedule (its row order, the rows never stored, its
// records), the factored schedule, and the per-position tables.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#include "host/pack_internal.h"
#include "host/pack_shared_sums.h"

namespace sk {
namespace {

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

// What the phases read about the example's DAG, by reference node id unless
// said otherwise.
struct XNodes {
  int nn = 0;
  // phase 1: level of every node (-1: leaf), the non-leaf nodes by (level,
  // reference index) and a node's place in that order (its level-order id)
  std::vector<int> level, order, nid;
  int nlev = 0, nl = 0;
  // phase 2: gamma (bit 0) / phi (bit 1) row flags, tested once (the later
  // phases ask repeatedly), and their (code, len) key's index
  std::vector<uint8_t> fl;
  std::vector<uint32_t> gix;
  std::vector<double> Pw;  // phase 3: number of root->v paths
  std::vector<int> npar;   // edges into v
};

bool fail_x(XOut& O, int rc, const char* msg) {
  O.err = msg;
  O.rc = rc;
  return false;
}

// phase 1 (children come first in reference numbering)
bool node_levels(const Example& X, XNodes& N, XOut& O) {
  const int nn = N.nn;
  N.level.assign(nn, -1);
  for (int v = 0; v < nn; ++v) {
    const uint32_t e0 = X.edge_off[v], e1 = X.edge_off[v + 1];
    if (e0 == e1) continue;  // leaf
    int lv = 0;
    bool any_leaf = false;
    for (uint32_t k = e0; k < e1; ++k) {
      const int c = N.level[X.edge_to[k]];
      if (c < 0) any_leaf = true;
      else lv = std::max(lv, c + 1);
    }
    if (any_leaf && e1 - e0 != 1) return fail_x(O, SK_ERR_INVALID, "unexpected DAG shape: stem with a leaf child");
    N.level[v] = lv;
    N.nlev = std::max(N.nlev, lv + 1);
  }
  {  // a counting sort
    std::vector<int> lstart(N.nlev + 1, 0);
    for (int v = 0; v < nn; ++v)
      if (N.level[v] >= 0) ++lstart[N.level[v] + 1];
    for (int l = 0; l < N.nlev; ++l) lstart[l + 1] += lstart[l];
    N.order.resize(lstart[N.nlev]);
    for (int v = 0; v < nn; ++v)
      if (N.level[v] >= 0) N.order[lstart[N.level[v]]++] = v;
  }
  N.nl = (int)N.order.size();
  if (N.nl >= 0xffff) return fail_x(O, SK_ERR_UNSUPPORTED, "example too large: more than 65534 non-leaf DAG nodes");
  N.nid.assign(nn, -1);
  for (int k = 0; k < N.nl; ++k) N.nid[N.order[k]] = k;
  return true;
}

// phase 2
void row_keys(const Example& X, const KeyTables& K, XNodes& N) {
  N.fl.assign(N.nn, 0);
  N.gix.assign(N.nn, 0);
  if (K.gam_on)
    for (int v = 0; v < N.nn; ++v) N.fl[v] |= is_gamma(X, v) ? 1 : 0;
  if (K.phi_on)
    for (int v = 0; v < N.nn; ++v) N.fl[v] |= is_phi(X, v) ? 2 : 0;
  for (int v = 0; v < N.nn; ++v)
    if (N.fl[v]) N.gix[v] = K.gamma_idx(gamma_key(X, v));
}

// phase 3 (parents have larger reference ids)
std::vector<double> path_weights(const Example& X) {
  const int nn = X.n_nodes();
  std::vector<double> Pw(nn, 0.0);
  for (uint32_t r : X.roots) Pw[r] += 1.0;
  for (int v = nn - 1; v >= 0; --v)
    for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k) Pw[X.edge_to[k]] += Pw[v];
  return Pw;
}

std::vector<int> parent_counts(const Example& X) {
  const int nn = X.n_nodes();
  std::vector<int> npar(nn, 0);
  for (int v = 0; v < nn; ++v)
    for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k) ++npar[X.edge_to[k]];
  return npar;
}

// phase 4: node, edge and bp-frequency records in level order, the levels'
// offsets, and whether the register-class kernel can take the example as a y
bool level_order_records(const Example& X, const XNodes& N, XOut& O) {
  const int nl = N.nl;
  for (auto* q : {&O.nd_a, &O.nd_b, &O.nd_c}) q->reserve(nl);
  O.nd_w.reserve(nl);
  O.nd_nbp.reserve(nl);
  O.nd_P.reserve(nl);
  O.ed.reserve((size_t)X.n_edges());
  O.bpf_code.reserve(X.bpf_off[N.nn]);
  O.bpf_p.reserve(X.bpf_off[N.nn]);
  bool big_gap = false;
  for (int k = 0; k < nl; ++k) {
    const int v = N.order[k];
    const uint32_t e0 = X.edge_off[v], e1 = X.edge_off[v + 1];
    const uint32_t b0 = X.bpf_off[v], b1 = X.bpf_off[v + 1];
    const bool loop = N.level[v] == 0;  // single leaf child
    const uint32_t eloc = (uint32_t)O.ed.size(), bloc = (uint32_t)O.bpf_code.size();
    const uint32_t ne = loop ? 0u : e1 - e0;
    if (eloc > 0xffff || bloc > 0xffff || ne > 0xff || b1 - b0 > 0xff || X.last[v] - X.first[v] > 0xffff)
      return fail_x(O, SK_ERR_UNSUPPORTED, "example too large for the 16-bit packed DAG layout");
    O.nd_a.push_back(eloc | (ne << 16) | ((b1 - b0) << 24));
    O.nd_b.push_back((X.last[v] - X.first[v]) | (bloc << 16));
    O.nd_c.push_back(loop ? X.edge_gaps[e0] : 0u);
    O.nd_w.push_back(X.weight[v]);
    O.nd_nbp.push_back(X.prof5[(size_t)X.first[v] * 5 + 4]);
    O.nd_P.push_back(N.Pw[v]);
    if (!loop) {
      for (uint32_t t = e0; t < e1; ++t) {
        const int c = N.nid[X.edge_to[t]];
        if (c < 0) return fail_x(O, SK_ERR_INVALID, "unexpected DAG shape: stem with a leaf child");
        if (X.edge_gaps[t] > 0xffff) return fail_x(O, SK_ERR_UNSUPPORTED, "gap count exceeds 65535");
        big_gap |= X.edge_gaps[t] > 1023;
        O.ed.push_back(make_uint2((uint32_t)c | (X.edge_gaps[t] << 16), (uint32_t)k));
      }
    }
    for (uint32_t t = b0; t < b1; ++t) {
      O.bpf_code.push_back(X.bpf_code[t]);
      O.bpf_p.push_back(X.bpf_p[t]);
    }
  }
  std::vector<int32_t> lv(N.nlev + 1, 0);
  for (int k = 0; k < nl; ++k) lv[N.level[N.order[k]] + 1]++;
  for (int l = 0; l < N.nlev; ++l) lv[l + 1] += lv[l];
  O.lvl.insert(O.lvl.end(), lv.begin(), lv.end());
  // the register-class kernel's y records: child:11 | parent:11 | gaps:10
  // (at most 2,047 nodes: every register class keeps its last slot free,
  // the dummy records' target, dag_stem.hip)
  O.nl = nl;
  O.big = nl > 2047 || big_gap;
  O.ex_big.push_back(O.big ? 1 : 0);
  return true;
}

// the record of row v in an x schedule: nch child records, its output slot
// (bpf_beg: in the level-order bpf array of this example, see nd_b)
XRow x_row(const Example& X, const XNodes& N, const XOut& O, int v, uint32_t nch, uint32_t slot, bool phi) {
  const uint32_t b0 = X.bpf_off[v], b1 = X.bpf_off[v + 1];
  XRow xr;
  xr.a = nch | ((b1 - b0) << 8) | ((N.level[v] == 0 ? X.edge_gaps[X.edge_off[v]] : 0u) << 16);
  xr.b = (X.last[v] - X.first[v]) | (slot << 16);
  xr.w = X.weight[v];
  xr.nbp = X.prof5[(size_t)X.first[v] * 5 + 4];
  xr.bp0 = b1 > b0 ? X.bpf_p[b0] : 0.0f;
  xr.P = N.Pw[v];
  xr.c = (O.nd_b[N.nid[v]] >> 16) | ((b1 > b0 ? (uint32_t)X.bpf_code[b0] : 0u) << 16) | (phi ? 0x80000000u : 0u);
  return xr;
}

// A schedule's HBM row slots: a row's slot is recycled once its last reader
// has been produced (a LIFO free list keeps hot addresses hot).
struct SlotPool {
  std::vector<uint32_t> free;
  int n = 0;  // slots handed out so far
  uint32_t take() {
    if (free.empty()) return (uint32_t)n++;
    const uint32_t s = free.back();
    free.pop_back();
    return s;
  }
  void give(uint32_t s) { free.push_back(s); }
};

// phase 5: the full x schedule, rows in reference (post-)order.  Rows nobody
// reads (roots) get no slot.
bool full_schedule(const Example& X, const XNodes& N, XOut& O) {
  const int nn = N.nn;
  O.xr_ch.reserve((size_t)X.n_edges());
  O.xrow.reserve(N.nl);
  O.xr_node.reserve(N.nl);
  std::vector<int> last_parent(nn, -1);
  for (int v = 0; v < nn; ++v)
    for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k)
      last_parent[X.edge_to[k]] = std::max(last_parent[X.edge_to[k]], v);
  std::vector<uint32_t> slot(nn, 0xffff);
  SlotPool pool;
  for (int v = 0; v < nn; ++v) {
    if (N.level[v] < 0) continue;
    const uint32_t e0 = X.edge_off[v], e1 = X.edge_off[v + 1];
    uint32_t nch = 0;
    if (N.level[v] != 0) {
      for (uint32_t k = e0; k < e1; ++k) {
        O.xr_ch.push_back(slot[X.edge_to[k]] | (X.edge_gaps[k] << 16));
        ++nch;
      }
    }
    for (uint32_t k = e0; k < e1; ++k) {
      const int c = X.edge_to[k];
      if (N.level[c] >= 0 && last_parent[c] == v && slot[c] != 0xffff) pool.give(slot[c]);
    }
    if (last_parent[v] >= 0) slot[v] = pool.take();
    O.xrow.push_back(x_row(X, N, O, v, nch, slot[v], false));
    O.xr_node.push_back((uint32_t)N.nid[v]);
  }
  if (pool.n >= 0xffff) return fail_x(O, SK_ERR_UNSUPPORTED, "too many live DAG rows");
  O.ex_nslots.push_back(pool.n);
  O.max_slots = std::max(O.max_slots, pool.n);
  return true;
}

// phase 6: the gamma schedule's row order (gamma rows included: they are
// skipped when the records are emitted).  A depth-first post-order whose
// last-visited child of a row is, where it can be, one that row alone reads
// among its first four records (stored nowhere: the row takes it from
// registers, never_stored), the reference numbering with SK_REF_ORDER; then
// each phi row moved to just before its first parent (it has no row
// children, so any earlier place is valid): the parent takes it from
// registers too (distance 1), and the row before it, usually a swept one,
// prefetches its first components.
std::vector<int> gamma_row_order(const Example& X, const XNodes& N, bool phi_on) {
  const int nn = N.nn;
  const std::vector<int>& level = N.level;
  const std::vector<uint8_t>& fl = N.fl;
  std::vector<int> cand(nn, -1);  // a row's register candidate
  for (int v = 0; v < nn; ++v) {
    if (level[v] <= 0 || (fl[v] & 2)) continue;
    for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1] && k < X.edge_off[v] + 4; ++k) {
      const int c = X.edge_to[k];
      if (N.npar[c] == 1 && level[c] >= 0 && !(fl[c] & 1)) {
        cand[v] = c;
        break;
      }
    }
  }
  std::vector<int> dfo;  // the post-order
  if (SK_KNOB("SK_REF_ORDER")) {
    for (int v = 0; v < nn; ++v)
      if (level[v] >= 0) dfo.push_back(v);
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
          dfo.push_back(v);
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
  for (int i = 0; i < (int)dfo.size(); ++i) pos[dfo[i]] = i;
  for (int v = 0; v < nn; ++v)
    for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k) {
      const int c = X.edge_to[k];
      if (pos[v] < nn && (first_parent[c] == nn || pos[v] < pos[first_parent[c]])) first_parent[c] = v;
    }
  // the phi rows moved before each row (first parent nn: the roots'),
  // in order, as one CSR list
  const bool move = phi_on && !SK_KNOB("SK_PHI_POSTORDER");
  std::vector<int> o1, boff(nn + 2, 0), bl;
  o1.reserve(dfo.size());
  for (int v : dfo) {
    if (move && (fl[v] & 2)) ++boff[first_parent[v] + 1];
    else o1.push_back(v);
  }
  for (int i = 0; i <= nn; ++i) boff[i + 1] += boff[i];
  bl.resize(boff[nn + 1]);
  {
    std::vector<int> bf(boff.begin(), boff.end() - 1);
    for (int v : dfo)
      if (move && (fl[v] & 2)) bl[bf[first_parent[v]]++] = v;
  }
  std::vector<int> o2;
  o2.reserve(dfo.size() + 8);
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
  return o2;
}

// phase 7: rows read only by the next row, among its first four children,
// are never stored: the next row takes them from registers (slot 0xfffe)
std::vector<uint8_t> never_stored(const Example& X, const XNodes& N, const std::vector<int>& gorder) {
  std::vector<uint8_t> nostore(N.nn, 0);
  if (SK_KNOB("SK_STORE_ALL")) return nostore;
  std::vector<int> emitted;
  for (int v : gorder)
    if (!(N.fl[v] & 1)) emitted.push_back(v);
  for (size_t i = 0; i + 1 < emitted.size(); ++i) {
    const int v = emitted[i], r = emitted[i + 1];
    if (N.npar[v] != 1 || N.level[r] <= 0 || N.level[v] < 0 || (N.fl[r] & 2)) continue;
    for (uint32_t k = X.edge_off[r]; k < X.edge_off[r + 1] && k < X.edge_off[r] + 4; ++k)
      if (X.edge_to[k] == v) nostore[v] = 1;
  }
  return nostore;
}

// a node's last parent in the order gorder (-1: none)
std::vector<int> last_readers(const Example& X, const std::vector<int>& gorder) {
  const int nn = X.n_nodes();
  std::vector<int> glast(nn, -1), gpos(nn, -1);
  for (int i = 0; i < (int)gorder.size(); ++i) gpos[gorder[i]] = i;
  for (int v : gorder)
    for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k) {
      const int c = X.edge_to[k];
      if (glast[c] < 0 || gpos[v] > gpos[glast[c]]) glast[c] = v;
    }
  return glast;
}

// the child records of gamma-schedule row v (no gamma row), appended to
// xg_ch / xg_clg / xg_cpf / xg_cty: a gamma child is a record 0x8000 | gamma
// index, its weight factors g^lg pf in xg_clg / xg_cpf.  Returns their count.
uint32_t gamma_row_children(const Example& X, const KeyTables& K, const XNodes& N,
                            const std::vector<uint32_t>& gslot, int v, XOut& O) {
  const uint32_t e0 = X.edge_off[v], e1 = X.edge_off[v + 1];
  auto rec = [&](uint32_t ch, uint32_t clg, float cpf, int ty) {
    O.xg_ch.push_back(ch);
    O.xg_clg.push_back(clg);
    O.xg_cpf.push_back(cpf);
    O.xg_cty.push_back((uint8_t)ty);
  };
  if (N.fl[v] & 2) {
    // components: per child c a Phi row (type 2) and its Gamma row
    // (type 4), then Gamma_{code,len} of the row itself (type 3)
    const uint32_t kp = gamma_key(X, v);
    for (uint32_t k = e0; k < e1; ++k) {
      const int c = X.edge_to[k];
      const uint32_t pi = K.phi_idx(kp, gamma_key(X, c));
      for (int ty : {2, 4})
        rec((ty == 2 ? 0x4000u | pi : 0x8000u | N.gix[c]) | (X.edge_gaps[k] << 16), X.edge_gaps[X.edge_off[c]],
            X.bpf_p[X.bpf_off[c]], ty);
      O.phk_idx.push_back(pi);
    }
    rec(0x8000u | N.gix[v], 0u, 0.0f, 3);
    O.gra_gidx.push_back(N.gix[v]);
    O.gra_row.push_back((uint32_t)O.xgrow.size());  // (+ the example's xgrow base)
    return 2 * (e1 - e0) + 1;
  }
  if (N.level[v] == 0) return 0;
  for (uint32_t k = e0; k < e1; ++k) {
    const int c = X.edge_to[k];
    if (N.fl[c] & 1)
      rec((0x8000u | N.gix[c]) | (X.edge_gaps[k] << 16), X.edge_gaps[X.edge_off[c]], X.bpf_p[X.bpf_off[c]], 1);
    else
      rec(gslot[c] | (X.edge_gaps[k] << 16), 0u, 1.0f, 0);
  }
  return e1 - e0;
}

// the input of the factored schedule: the gamma schedule's rows with their
// child records by identity, and the phi rows among them (by input row)
struct SsInput {
  std::vector<SsRow> rows;
  std::vector<uint32_t> gra;
  std::vector<int32_t> row_of;  // node -> its input row
  uint32_t next_key = 0;        // identities of the phi rows' components (never shared)
};
// row v, whose record is xr and whose child records begin at xg_ch[rec0]
void ss_add_row(const Example& X, const XNodes& N, const XOut& O, int v, const XRow& xr, size_t rec0, SsInput& ss) {
  const bool phi = (N.fl[v] & 2) != 0, loop = N.level[v] == 0;
  SsRow W;
  W.xr = xr;
  W.node = (uint32_t)N.nid[v];
  W.user = W.swept = !phi && !loop;
  size_t t = rec0;
  auto table = [&](uint32_t key) {
    W.rec.push_back(SsRec{-1, key, O.xg_ch[t] & 0xffffu, O.xg_ch[t] >> 16, O.xg_clg[t], O.xg_cpf[t], O.xg_cty[t]});
    ++t;
  };
  if (phi) {
    for (; t < O.xg_ch.size();) table(ss.next_key++);
    ss.gra.push_back((uint32_t)O.xgrow.size());
  } else if (!loop) {
    for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k) {
      const int c = X.edge_to[k];
      if (N.fl[c] & 1) {
        table((uint32_t)c);
      } else {
        W.rec.push_back(SsRec{ss.row_of[c], 0u, 0u, X.edge_gaps[k], 0u, 1.0f, 0});
        ++t;
      }
    }
  }
  ss.row_of[v] = (int32_t)O.xgrow.size();
  ss.rows.push_back(std::move(W));
}

// phase 8: the gamma schedule's records in the order gorder -- the gamma
// rows' K inputs (gr_*), the other rows with slots among themselves -- and,
// where ss is given, the same rows as the input of the factored schedule.
// Returns the slots used.
int gamma_schedule(const Example& X, const KeyTables& K, const XNodes& N, const std::vector<int>& gorder,
                   const std::vector<uint8_t>& nostore, XOut& O, SsInput* ss) {
  const int nn = N.nn;
  const size_t ne_x = (size_t)X.n_edges();
  O.xgrow.reserve(N.nl);
  O.xg_node.reserve(N.nl);
  O.xg_ch.reserve(2 * ne_x + N.nl);
  O.xg_clg.reserve(2 * ne_x + N.nl);
  O.xg_cpf.reserve(2 * ne_x + N.nl);
  O.xg_cty.reserve(2 * ne_x + N.nl);
  // each row's slot is freed at its last parent in this order
  const std::vector<int> glast = last_readers(X, gorder);
  std::vector<uint32_t> gslot(nn, 0xffff);
  SlotPool pool;
  if (ss) {
    ss->rows.reserve(gorder.size());
    ss->row_of.assign(nn, -1);
    ss->next_key = (uint32_t)nn;
  }
  int nlxg = 0;
  for (int v : gorder) {
    const uint32_t e0 = X.edge_off[v], e1 = X.edge_off[v + 1];
    if (N.fl[v] & 1) {
      O.gr_info.push_back(N.gix[v] | (X.edge_gaps[e0] << 16));
      O.gr_pf.push_back(X.bpf_p[X.bpf_off[v]]);
      O.gr_P.push_back(N.Pw[v]);
      continue;
    }
    const size_t rec0 = O.xg_ch.size();
    const uint32_t nch = gamma_row_children(X, K, N, gslot, v, O);
    for (uint32_t k = e0; k < e1; ++k) {
      const int c = X.edge_to[k];
      if (N.level[c] >= 0 && glast[c] == v && gslot[c] < 0x4000) {
        pool.give(gslot[c]);
        gslot[c] |= 0x10000;  // freed (a second edge to c must not free it again)
      }
    }
    if (nostore[v]) gslot[v] = 0xfffe;
    else if (N.npar[v] > 0) gslot[v] = pool.take();
    const XRow xr = x_row(X, N, O, v, nch, gslot[v], (N.fl[v] & 2) != 0);
    if (ss) ss_add_row(X, N, O, v, xr, rec0, *ss);
    O.xgrow.push_back(xr);
    O.xg_node.push_back((uint32_t)N.nid[v]);
    ++nlxg;
  }
  if (K.phi_on) {  // this example's phi keys as a bitset (items take unions)
    const size_t W = (K.phi_raw.size() + 63) / 64;
    O.ex_phi_bits.assign(W, 0ull);
    for (size_t j = 0; j < O.phk_idx.size(); ++j) O.ex_phi_bits[O.phk_idx[j] / 64] |= 1ull << (O.phk_idx[j] % 64);
  }
  O.ex_nlxg.push_back(nlxg);
  return pool.n;
}

// phase 9: the factored schedule of the rows in ss, or, over a limit of the
// layout, this example's plain rows again
void factored_schedule(const KeyTables& K, SsInput&& ss, XOut& O) {
  SsOut F;
  if (shared_sums_schedule(std::move(ss.rows), K.ss_thr, SK_KNOB("SK_STORE_ALL") != nullptr, F)) {
    O.xf_row.swap(F.row);
    O.xf_node.swap(F.node);
    O.xf_ch.swap(F.ch);
    O.xf_clg.swap(F.clg);
    O.xf_cpf.swap(F.cpf);
    O.xf_cty.swap(F.cty);
    for (uint32_t r : ss.gra) O.xf_gra_row.push_back(F.new_index[r]);  // (+ the example's base)
    O.ss_rows = F.n_shared;
    O.ss_repl = F.n_replaced;
    O.max_slots = std::max(O.max_slots, F.nslots);
  } else {
    O.xf_row = O.xgrow;
    O.xf_node = O.xg_node;
    O.xf_ch = O.xg_ch;
    O.xf_clg = O.xg_clg;
    O.xf_cpf = O.xg_cpf;
    O.xf_cty = O.xg_cty;
    O.xf_gra_row = O.gra_row;
  }
}

// phase 10: the per-example scalars, the per-position tables and the flags
// of the string and BPLA kernels' fast paths
void position_tables(const Example& X, const XNodes& N, XOut& O) {
  {  // y role: no gap column in any non-leaf node (the Gamma rows need it)
    bool gl = true;
    for (int k = 0; k < N.nl; ++k) gl &= O.nd_nbp[k] == 0.0f;
    O.ex_gapless.push_back(gl ? 1 : 0);
  }
  O.ex_nl.push_back(N.nl);
  O.ex_nlev.push_back(N.nlev);
  O.nlev = N.nlev;
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

}  // namespace

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

void pack_x(const Example& X, const KeyTables& K, XOut& O) {
  XNodes N;
  N.nn = X.n_nodes();
  if (!node_levels(X, N, O)) return;
  row_keys(X, K, N);
  N.Pw = path_weights(X);
  N.npar = parent_counts(X);
  // (the y-role records are formed after the x-role pass: pack_y)
  if (!level_order_records(X, N, O)) return;
  if (!full_schedule(X, N, O)) return;
  // the gamma schedule: the same rows without the gamma rows, in an order of
  // its own, slots only among the remaining rows
  const std::vector<int> gorder = gamma_row_order(X, N, K.phi_on);
  const std::vector<uint8_t> nostore = never_stored(X, N, gorder);
  SsInput ss;
  const int gslots = gamma_schedule(X, K, N, gorder, nostore, O, K.ss_on ? &ss : nullptr);
  if (K.ss_on) factored_schedule(K, std::move(ss), O);
  if (gslots >= 0x4000) {  // slot ids share the record with the gamma / phi flags
    fail_x(O, SK_ERR_UNSUPPORTED, "too many live DAG rows");
    return;
  }
  O.max_slots = std::max(O.max_slots, gslots);
  O.n_nostore = (int)std::count(nostore.begin(), nostore.end(), 1);
  O.n_nodes = N.nn;
  O.gslots = gslots;
  position_tables(X, N, O);
}

}  // namespace sk
