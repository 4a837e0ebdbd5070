// Planner of the DAG stem kernel (kernels/dag_stem.hip, dag_stem_big.hip) and
// the string kernels (kernels/profile_string.hip): the kinds Su / Si / LSu
// stem, string and stem + string.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host/runtime_types.h"
#include "ribosum85_60.inc"

namespace sk {
namespace {

// ---- host-side work lists
// stem items: pairs grouped by y, chunks, largest first, in classes by the
// y example's register template (MAXK = 64-node slots per lane): one
// launch per class, each sized (LDS, waves) for its own largest y
struct StemClass {
  int maxk = 0;
  int max_nl = 0, max_edges = 0, max_bpf = 0, max_nch = 0;
  int nwaves = 1, grid = 1;
  size_t item_off = 0, n_items = 0;
  size_t slot_off = 0, n_slots = 0;         // the class's Gamma table slots in slot_y
  bool gam_shared = false;                  // one Gamma table per y (else per workgroup)
  bool phi_shared = false;                  // ... and one Phi table per y (else per workgroup and item)
  int32_t queue_off[sk::kStemQueues + 1] = {};  // the item queues' ranges, from item_off
  size_t tab_off = 0;                       // its tables in the scratch's table region (doubles)
};
// what plan_stem_items gives run_dag_pairs
struct StemPlan {
  std::vector<StemClass> classes;
  std::vector<int4> items;
  std::vector<int32_t> slot_y;  // Gamma table slot -> y, class by class
  std::vector<int32_t> ixs;
  std::vector<int64_t> ioidx;
  std::vector<int32_t> big_x, big_y;  // pairs whose y goes to the big-y kernel
  std::vector<int64_t> big_o;
  int big_max_nl = 0;
  double cells = 0.0;  // sum of |x| * |y| over the pairs (sk_last_timing)
};

// (host only but for the kernels' attributes, sk::stem_kernel_attr: that call
// can fail, so the status is returned and the plan filled in place, where
// order_str_pairs, which cannot fail, returns its struct.  Of the context it
// reads n_cu and, on an error, sets the message: no last_* field.)
int plan_stem_items(sk_context* ctx, const HostPack& PX, const HostPack& PY, const int32_t* x, const int32_t* y,
                    int64_t n, int ny, int max_len, StemPlan& plan) {
  std::vector<int64_t> cnt(ny + 1, 0);
  for (int64_t k = 0; k < n; ++k) cnt[y[k] + 1]++;
  for (int j = 0; j < ny; ++j) cnt[j + 1] += cnt[j];
  std::vector<int64_t> byy(n);
  {
    std::vector<int64_t> pos(cnt.begin(), cnt.end() - 1);
    for (int64_t k = 0; k < n; ++k) byy[pos[y[k]]++] = k;
  }
  // within one y, costliest x first: the waves of a workgroup take the
  // item's pairs round-robin, so equal-cost rounds and a cheap last round
  // (one packed key per pair, ties by input order: deterministic)
  // (the y's on host threads: each sorts its own range of byy)
  {
    std::atomic<int> nextj{0};
    auto work = [&]() {
      std::vector<uint64_t> key;
      std::vector<int64_t> tmp;
      for (int j = nextj.fetch_add(1); j < ny; j = nextj.fetch_add(1)) {
        const int64_t b = cnt[j], e = cnt[j + 1];
        if (e - b < 2) continue;
        key.resize(e - b);
        for (int64_t t = b; t < e; ++t)
          key[t - b] = ((uint64_t)(0xffffffffu - (uint32_t)PX.ex_nl[x[byy[t]]]) << 32) | (uint32_t)(t - b);
        std::sort(key.begin(), key.end());
        tmp.assign(byy.begin() + b, byy.begin() + e);
        for (int64_t t = b; t < e; ++t) byy[t] = tmp[(uint32_t)key[t - b]];
      }
    };
    run_pool(plan_threads(n / 65536 + 1), work);
  }
  plan.ixs.resize(n);
  plan.ioidx.resize(n);
  for (int64_t t = 0; t < n; ++t) {
    plan.ixs[t] = x[byy[t]];
    plan.ioidx[t] = byy[t];
  }
  // y examples beyond the register classes (or forced there by the
  // diagnostic SK_FORCE_BIG_Y=1) go to sk_dag_stem_big_kernel
  const bool force_big = [] {
    const char* e = SK_KNOB("SK_FORCE_BIG_Y");
    return e && std::atoi(e) != 0;
  }();
  std::vector<uint8_t> ybig(ny, 0);
  for (int j = 0; j < ny; ++j) ybig[j] = force_big || PY.ex_big[j] ? 1 : 0;
  auto in_class = [&](int j, int maxk) {
    return !ybig[j] && sk::stem_maxk(PY.ex_nl[j] + 1) == maxk;  // (one slot free: dag_stem.hip zslot)
  };
  {
    std::vector<int64_t> bk;  // pairs dealt cyclically to the waves: costliest first
    for (int j = 0; j < ny; ++j) {
      if (!ybig[j] || cnt[j + 1] == cnt[j]) continue;
      plan.big_max_nl = std::max(plan.big_max_nl, PY.ex_nl[j]);
      for (int64_t t = cnt[j]; t < cnt[j + 1]; ++t) bk.push_back(byy[t]);
    }
    std::stable_sort(bk.begin(), bk.end(), [&](int64_t a, int64_t b) {
      return (double)PX.ex_nl[x[a]] * PY.ex_nl[y[a]] > (double)PX.ex_nl[x[b]] * PY.ex_nl[y[b]];
    });
    for (int64_t k : bk) {
      plan.big_x.push_back(x[k]);
      plan.big_y.push_back(y[k]);
      plan.big_o.push_back(k);
    }
  }
  for (int maxk : {32, 28, 24, 20, 17, 16, 12, 8, 4}) {
    StemClass C;
    C.maxk = maxk;
    C.slot_off = plan.slot_y.size();
    bool any = false;
    for (int j = 0; j < ny; ++j) {
      if (cnt[j + 1] == cnt[j] || !in_class(j, maxk)) continue;
      any = true;
      C.max_nl = std::max(C.max_nl, PY.ex_nl[j]);
      C.max_edges = std::max(C.max_edges, PY.ex_edge_base[j + 1] - PY.ex_edge_base[j]);
      C.max_bpf = std::max(C.max_bpf, PY.ex_bpf_base[j + 1] - PY.ex_bpf_base[j]);
      C.max_nch = std::max(C.max_nch, PY.ex_nch[j]);
    }
    if (!any) continue;
    sk::StemLaunch L;
    L.lds_max_nl = 64 * maxk;
    L.lds_max_edges = (C.max_edges + 3) & ~3;
    L.lds_max_bpf = (C.max_bpf + 1 + 3) & ~3;
    L.lds_max_nch = C.max_nch + 2;  // + 2 dummy chunks read past the end (dag_stem.hip)
    L.lds_max_len_pad = (max_len + 2 + 3) & ~3;
    L.n_gpow = max_len + 2;
    L.n_gpow_pad = (L.n_gpow + 1) & ~1;
    L.xset.n_gam = (int32_t)PX.gam_key.size();
    L.gam_on = L.xset.n_gam > 0;
    int max_dyn = 0, vgprs = 0, max_w = 8;
    SK_HIP(ctx, sk::stem_kernel_attr(L.lds_max_nl, &max_dyn, &vgprs, &max_w));
    const int valloc = ((std::max(vgprs, 1) + 7) / 8) * 8;
    const int waves_cu_vgpr = 4 * std::min(8, 512 / valloc);
    int best = 0, per_cu = 1;
    for (int w = max_w; w >= 1; --w) {  // the template's __launch_bounds__
      const size_t lds = sk::stem_lds_bytes(L, w);
      if (lds > (size_t)max_dyn) continue;
      const int pc = std::min<int>((int)(163840 / lds), std::min(32, waves_cu_vgpr) / w);
      if (pc * w > best) {
        best = pc * w;
        C.nwaves = w;
        per_cu = pc;
      }
    }
    if (best == 0) return fail(ctx, SK_ERR_UNSUPPORTED, "y example too large for LDS");
    C.grid = ctx->n_cu * per_cu;
    // Work items = pairs of one y (the workgroup stages one y DAG in LDS
    // and waits for its slowest wave at every item boundary, about half a
    // pair per wave).  Whole y columns are dealt to eight item queues, one
    // per XCD (the workgroups blockIdx.x % 8 == q pull from queue q and
    // share an L2: the fewer y's they are on at a time, the more of the
    // Gamma, Phi and node-record reads hit it): by cost, largest first onto
    // the least-loaded queue, a queue's columns in that order.  Inside a
    // queue, guided self-scheduling: each item is 1/(K * grid / 8) of the
    // queue's remaining cost (at least one round of W pairs), so the first
    // items are large (few boundaries) and the last ones a round each (short
    // launch tail) -- and at most 1/8 of its column's cost, so that the
    // queue's workgroups stand on a few y's, not on one each.  (K = 1.5; NS
    // 161k pairs/s at K = 1, 160.8k at 1.5, 160.0k at 2, 157.2k at 8; C2
    // 148k at 1.5, 140k at 1.)  A workgroup whose queue is empty takes from
    // the others (dag_stem.hip).
    // A gapless y of a launch with gamma keys gets a table slot (Gamma and
    // Phi), carried in its items' .w (-1: none).
    std::vector<int> ysel;
    std::vector<double> ycost(ny, 0.0);
    for (int j = 0; j < ny; ++j) {
      if (cnt[j + 1] == cnt[j] || !in_class(j, maxk)) continue;
      ysel.push_back(j);
      for (int64_t t = cnt[j]; t < cnt[j + 1]; ++t)
        ycost[j] += (double)PX.ex_nl[x[byy[t]]] * (double)PY.ex_nl[j];
    }
    std::stable_sort(ysel.begin(), ysel.end(), [&](int a, int b) {
      return cnt[a + 1] - cnt[a] > cnt[b + 1] - cnt[b];
    });
    double gss_k = 1.5;  // tuning knob: SK_GSS_K (items per workgroup at the start)
    if (const char* e = SK_KNOB("SK_GSS_K")) gss_k = std::max(0.25, std::atof(e));
    int nq = sk::kStemQueues;  // SK_ITEM_QUEUES=1: one queue, uncapped items
    if (const char* e = SK_KNOB("SK_ITEM_QUEUES")) nq = std::min(std::max(std::atoi(e), 1), sk::kStemQueues);
    double cap = nq > 1 ? 1.0 / 8.0 : 1.0;  // an item's largest share of its column (SK_ITEM_CAP: 1 / share)
    if (const char* e = SK_KNOB("SK_ITEM_CAP")) cap = 1.0 / std::max(1.0, std::atof(e));
    std::vector<int> qof(ny, 0);  // column -> queue
    double class_cost = 0.0;
    {
      std::vector<int> bycost(ysel);
      if (nq > 1)
        std::stable_sort(bycost.begin(), bycost.end(), [&](int a, int b) { return ycost[a] > ycost[b]; });
      std::vector<double> load(nq, 0.0);
      for (int j : bycost) {
        const int q = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        qof[j] = q;
        load[q] += ycost[j];
        class_cost += ycost[j];
      }
    }
    // the items in the class's one guided order (their sizes fall over the
    // whole launch, so every queue ends in short items and the workgroups
    // that come over from an empty queue find a fine-grained tail), each
    // into its column's queue
    std::vector<std::vector<int4>> qitems(nq);
    const double share = 1.0 / (gss_k * (double)C.grid);
    double remaining = class_cost;
    for (int j : ysel) {
      const double yw = (double)PY.ex_nl[j];
      int slot = -1;
      if (L.gam_on && PY.ex_gapless[j]) {
        slot = (int)(plan.slot_y.size() - C.slot_off);
        plan.slot_y.push_back(j);
      }
      int64_t b = cnt[j];
      while (b < cnt[j + 1]) {
        const double target = std::min(remaining * share, ycost[j] * cap);
        int64_t e = b;
        double cost = 0.0;
        // whole rounds of W pairs until the target cost is reached
        while (e < cnt[j + 1] && (e - b < C.nwaves || cost < target)) {
          const int64_t re = std::min<int64_t>(cnt[j + 1], e + C.nwaves);
          for (int64_t t = e; t < re; ++t) cost += (double)PX.ex_nl[x[byy[t]]] * yw;
          e = re;
        }
        qitems[qof[j]].push_back(make_int4(j, (int)b, (int)(e - b), slot));
        remaining -= cost;
        b = e;
      }
    }
    C.item_off = plan.items.size();
    for (int q = 0; q < sk::kStemQueues; ++q) {
      C.queue_off[q] = (int32_t)(plan.items.size() - C.item_off);
      if (q < nq) plan.items.insert(plan.items.end(), qitems[q].begin(), qitems[q].end());
    }
    C.queue_off[sk::kStemQueues] = (int32_t)(plan.items.size() - C.item_off);
    C.n_slots = plan.slot_y.size() - C.slot_off;
    C.n_items = plan.items.size() - C.item_off;
    C.grid = (int)std::min<int64_t>(C.grid, std::max<int64_t>(1, (int64_t)C.n_items));
    plan.classes.push_back(C);
  }
  double cells = 0.0;
  for (int64_t k = 0; k < n; ++k) cells += (double)PX.ex_nl[x[k]] * (double)PY.ex_nl[y[k]];
  plan.cells = cells;
  return SK_OK;
}

// string kernel: pairs of dyadic, never-empty profiles (both weighted or
// neither) take the fast path (profile_string.hip), first; the rest the
// general kernel, the permutation undone through oidx
// (one-hot pairs first, then the other fast pairs, then the rest)
// what order_str_pairs gives run_dag_pairs (spx empty: the pairs as given)
struct StrPlan {
  std::vector<int32_t> spx, spy;
  std::vector<int64_t> soidx;
  int64_t n_soh = 0, n_sfast = 0;  // one-hot pairs; fast pairs (one-hot included)
};

StrPlan order_str_pairs(const HostPack& PX, const HostPack& PY, const sk_kernel_params* kp, bool str,
                        const int32_t* x, const int32_t* y, int64_t n) {
  StrPlan plan;
  // (the fast kernels' per-wave LDS rows must fit a CU: else the general one)
  const int str_lds_len = (std::max(PY.max_len, 64) + 1) & ~1;
  if (str && kp->kind != SK_NAIVE_STR && !SK_KNOB("SK_STR_GENERAL") &&
      sk::str_fast_wave_lds_bytes(str_lds_len, false) + sk::kStrFastLds0 <= 163840) {
    auto cat = [&](int64_t k) {
      const int a = x[k], b = y[k];
      if (PX.ex_has_w[a] != PY.ex_has_w[b]) return 2;
      if (PX.ex_onehot[a] && PY.ex_onehot[b]) return 0;
      return PX.ex_str_fast[a] && PY.ex_str_fast[b] ? 1 : 2;
    };
    int64_t cnt3[3] = {0, 0, 0};
    for (int64_t k = 0; k < n; ++k) ++cnt3[cat(k)];
    plan.n_soh = cnt3[0];
    plan.n_sfast = cnt3[0] + cnt3[1];
    if (cnt3[0] != n && cnt3[1] != n && cnt3[2] != n) {
      plan.spx.reserve(n);
      plan.spy.reserve(n);
      plan.soidx.reserve(n);
      for (int c = 0; c < 3; ++c)
        for (int64_t k = 0; k < n; ++k)
          if (cat(k) == c) {
            plan.spx.push_back(x[k]);
            plan.spy.push_back(y[k]);
            plan.soidx.push_back(k);
          }
    }
  }
  return plan;
}

}  // namespace

// The DAG stem and string kinds of run_pairs (sk_api.cpp), which has checked
// the arguments and begun the call.
int run_dag_pairs(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
                      const int32_t* x, const int32_t* y, int64_t n, double* out_dev) {
  int rc = SK_OK;
  const int ny = (int)ys_->ex.size();
  const bool stem = kind_has_stem(kp->kind), str = kind_has_str(kp->kind);
  const HostPack& PX = xs_->pack;
  const HostPack& PY = ys_->pack;
  // SK_HOST_STATS: host planning time per phase (diagnostic)
  const bool host_stats = std::getenv("SK_HOST_STATS") != nullptr;
  auto now_ms = [] {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
  };
  const double th0 = host_stats ? now_ms() : 0.0;
  double th1 = th0, th2 = th0;

  StemPlan plan;
  const int max_len = std::max(PX.max_len, PY.max_len);
  if (stem) {
    rc = plan_stem_items(ctx, PX, PY, x, y, n, ny, max_len, plan);
    if (rc) return rc;
    ctx->last_cells = plan.cells;
  }

  if (host_stats) th1 = now_ms();
  std::vector<int32_t> item_phi_off, item_phi;
  const bool phi_on = stem && !PX.phi_al.empty() && !PX.gam_key.empty();
  bool two_streams = false;
  double *scratch_cls = nullptr, *scratch_tab = nullptr;
  int64_t big_stride = 0, big_wave = 0;
  int big_grid = 0;
  if (stem) {
    // class c runs on the main stream (c even) or the class stream (c odd):
    // one scratch region per stream, serving its classes in turn
    two_streams = plan.classes.size() > 1 && !SK_KNOB("SK_SERIAL_CLASSES");
    size_t scratch_need = 0, scratch_x = 0;
    // The Gamma and Phi tables of a class launch: one of each per gapless y
    // of the launch, written by the table kernel and read by every workgroup
    // on that y, if they fit a budget taken from free memory (a quarter of
    // it, the scratch held so far counted as free, 8 GiB at most;
    // SK_GAM_TABLE_MB: the budget in MB, 0 = never): first the Gamma tables
    // of the call's classes, in class order, then with what is left their
    // Phi tables (every phi key of the x set: n_phi rows per y, 11 MB for an
    // NS y; SK_PHI_TABLE_MB: their own budget in MB); else one per workgroup,
    // rebuilt per item (the Phi tables only behind shared Gamma tables).
    // The table kernels of all classes run first (below), so every class has
    // table memory of its own, past the two streams' regions.  Free memory is
    // asked for only when the tables do not fit the scratch the context
    // already holds, and if the scratch cannot be had with them, the call
    // goes on without (below).
    size_t tab_total = 0;
    size_t phi_budget = SIZE_MAX;
    if (const char* e = SK_KNOB("SK_PHI_TABLE_MB")) phi_budget = (size_t)std::max(0.0, std::atof(e) * 1048576.0);
    auto size_classes = [&](size_t gam_budget) {
      scratch_need = scratch_x = tab_total = 0;
      // the Gamma tables: per y of the launch (and their sums), or per workgroup
      auto gam_bytes = [&](const StemClass& C) {
        return C.n_slots * (size_t)PX.gam_key.size() * (size_t)(64 * C.maxk + 1) * sizeof(double);
      };
      // the Phi tables and sums likewise
      auto phi_bytes = [&](const StemClass& C) {
        return phi_on ? C.n_slots * (size_t)PX.phi_al.size() * (size_t)(64 * C.maxk + 1) * sizeof(double) : 0;
      };
      size_t total = 0, phi_total = 0;
      for (StemClass& C : plan.classes) {
        C.gam_shared = C.n_slots > 0 && total + gam_bytes(C) <= gam_budget;
        if (C.gam_shared) total += gam_bytes(C);
      }
      for (StemClass& C : plan.classes) {
        C.phi_shared = phi_on && C.gam_shared && total + phi_bytes(C) <= gam_budget &&
                       phi_total + phi_bytes(C) <= phi_budget;
        if (C.phi_shared) {
          total += phi_bytes(C);
          phi_total += phi_bytes(C);
        }
      }
      for (size_t c = 0; c < plan.classes.size(); ++c) {
        StemClass& C = plan.classes[c];
        if (C.gam_shared) {
          C.tab_off = tab_total / sizeof(double);
          tab_total += gam_bytes(C) + (C.phi_shared ? phi_bytes(C) : 0);
        }
        // + one junk row: root rows are stored there (never read)
        const int64_t slab = (int64_t)(PX.max_slots + 1) * 64 * C.maxk;
        const int64_t gtab1 = (int64_t)PX.gam_key.size() * 64 * C.maxk;
        const int64_t ptab = phi_on ? (int64_t)PX.phi_al.size() * (64 * C.maxk + 1) : 0;
        const size_t b = (size_t)C.grid *
                         (C.nwaves * slab + (C.phi_shared ? 0 : ptab) + (C.gam_shared ? 0 : gtab1)) * sizeof(double);
        size_t& r = (two_streams && (c & 1)) ? scratch_x : scratch_need;
        r = std::max(r, b);
      }
    };
    const bool any_slots = !PX.gam_key.empty() && !plan.slot_y.empty();
    size_classes(any_slots ? SIZE_MAX : 0);
    if (const char* e = SK_KNOB("SK_GAM_TABLE_MB")) {
      size_classes((size_t)std::max(0.0, std::atof(e) * 1048576.0));
    } else if (tab_total > 0 && scratch_need + scratch_x + tab_total + 512 > ctx->scratch_bytes) {
      size_t free_b = 0, total_b = 0;
      SK_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
      size_classes(std::min<size_t>((free_b + ctx->scratch_bytes) / 4, (size_t)8 << 30));
    }
    // big-y kernel: per wave S, G1 and the G0 slots, rows of `big_stride`
    // doubles; as many waves as pairs, the grid, and a scratch budget allow
    big_stride = ((int64_t)std::max(plan.big_max_nl, 1) + 63) / 64 * 64;
    big_wave = (int64_t)(PX.max_slots + 2) * big_stride;
    if (!plan.big_x.empty()) {
      size_t free_b = 0, total_b = 0;
      SK_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
      const size_t budget = std::max<size_t>(std::min<size_t>(free_b / 2, (size_t)32 << 30),
                                             (size_t)big_wave * 8 * sk::kStemBigWaves);
      const int64_t by_mem = (int64_t)(budget / ((size_t)big_wave * 8 * sk::kStemBigWaves));
      const int64_t by_pairs = ((int64_t)plan.big_x.size() + sk::kStemBigWaves - 1) / sk::kStemBigWaves;
      big_grid = (int)std::max<int64_t>(1, std::min<int64_t>({by_mem, by_pairs, (int64_t)ctx->n_cu * 8}));
      scratch_need = std::max(scratch_need,
                              (size_t)big_grid * sk::kStemBigWaves * (size_t)big_wave * sizeof(double));
    }
    const size_t big_need = scratch_need;  // (>= the classes' need on the main stream)
    auto get_scratch = [&]() {
      scratch_need = (std::max(scratch_need, big_need) + 255) / 256 * 256;
      scratch_x = (scratch_x + 255) / 256 * 256;
      return ensure_scratch(ctx, std::max<size_t>(scratch_need + scratch_x + tab_total, 64));
    };
    rc = get_scratch();
    if (rc && tab_total > 0) {  // not with the shared tables: per-workgroup tables then
      (void)hipGetLastError();
      size_classes(0);
      rc = get_scratch();
    }
    if (rc) return rc;
    scratch_cls = ctx->scratch + scratch_need / sizeof(double);
    scratch_tab = scratch_cls + scratch_x / sizeof(double);
  }
  // the items' phi keys (the union over their x's; gapless y only), for the
  // workgroups' Phi tables (dag_stem.hip) of the class launches that do not
  // share theirs (none otherwise: no unions, no uploads)
  bool phi_items = false;
  for (const StemClass& C : plan.classes) phi_items = phi_items || (phi_on && !C.phi_shared);
  if (phi_items) {
    // union of the x's key bitsets, keys ordered by gamma key (the kernel
    // forms one H row per gamma key and wave)
    // (contiguous item ranges on host threads, concatenated in item order)
    const size_t W = (PX.phi_al.size() + 63) / 64;
    const size_t ni = plan.items.size();
    std::vector<uint8_t> own(ni, 0);  // items of launches with per-workgroup Phi tables
    for (const StemClass& C : plan.classes)
      if (!C.phi_shared) std::fill(own.begin() + C.item_off, own.begin() + C.item_off + C.n_items, 1);
    const int T = plan_threads((int)(ni / 512 + 1));
    std::vector<std::vector<int32_t>> tkeys(T), tcnt(T);
    run_slices(T, [&](int t) {
      std::vector<uint64_t> acc(W);
      for (size_t i = ni * t / T; i < ni * (t + 1) / T; ++i) {
        const int4 it = plan.items[i];
        const size_t k0 = tkeys[t].size();
        if (own[i] && PY.ex_gapless[it.x]) {
          std::fill(acc.begin(), acc.end(), 0ull);
          for (int u = it.y; u < it.y + it.z; ++u) {
            const uint64_t* b = PX.ex_phi_bits.data() + (size_t)plan.ixs[u] * W;
            for (size_t w = 0; w < W; ++w) acc[w] |= b[w];
          }
          // (phi keys are numbered in gamma key order: the bits come sorted)
          for (size_t w = 0; w < W; ++w)
            for (uint64_t m = acc[w]; m; m &= m - 1) tkeys[t].push_back((int32_t)(w * 64 + __builtin_ctzll(m)));
        }
        tcnt[t].push_back((int32_t)(tkeys[t].size() - k0));
      }
    });
    item_phi_off.assign(1, 0);
    for (int t = 0; t < T; ++t) {
      item_phi.insert(item_phi.end(), tkeys[t].begin(), tkeys[t].end());
      for (int32_t c : tcnt[t]) item_phi_off.push_back(item_phi_off.back() + c);
    }
  }
  if (phi_on && std::getenv("SK_PHI_STATS")) {
    size_t shared = 0, slots = 0;
    for (const StemClass& C : plan.classes) {
      shared += C.phi_shared ? 1 : 0;
      slots += C.phi_shared ? C.n_slots : 0;
    }
    std::fprintf(stderr, "[phi] keys=%zu items=%zu item keys=%zu pairs=%lld phi components=%zu rows=%zu "
                 "classes=%zu sharing=%zu tables=%zu\n",
                 PX.phi_al.size(), plan.items.size(), item_phi.size(), (long long)n, PX.phk_idx.size(),
                 PX.run_rows().size(), plan.classes.size(), shared, slots);
  }

  if (host_stats) th2 = now_ms();
  const StrPlan splan = order_str_pairs(PX, PY, kp, str, x, y, n);
  const size_t n_str_pos = splan.n_sfast ? PX.pos_prof.size() + (ys_ == xs_ ? 0 : PY.pos_prof.size()) : 0;

  // ---- device work arena
  const size_t nb = (size_t)n;
  size_t need = 0;
  need += splan.soidx.size() * 8 + n_str_pos * (2 * sizeof(sk::StrPos) + sizeof(sk::StrCode)) + 1024;
  need += (item_phi_off.size() + item_phi.size()) * 4 + 512;
  // (the string fast kernels read gap^lane for every lane of a wave: 64 powers at least)
  const int n_gp_str = std::max(max_len + 4, 64);
  need += 256 * 8 + 16 * 8 + (size_t)(max_len + 4) * 8 + (size_t)n_gp_str * 8;
  need += 1024 + 256;
  need += plan.items.size() * sizeof(int4) + nb * (4 + 8) + nb * 8 * 2 + nb * 4 * 2 + 64 + 8 * 256;
  need += plan.slot_y.size() * 4 + 256;
  need += plan.big_x.size() * (4 + 4 + 8) + 3 * 256;
  need += 16 * 256;
  rc = ensure_work(ctx, need);
  if (rc) return rc;
  Arena A{static_cast<char*>(ctx->work), 0, ctx->work_bytes};
  double* d_co = A.take<double>(256);
  double* d_gp_loop = A.take<double>(max_len + 4);
  double* d_st = A.take<double>(16);
  double* d_gp_str = A.take<double>(n_gp_str);
  int4* d_items = A.take<int4>(std::max<size_t>(plan.items.size(), 1));
  int32_t* d_ixs = A.take<int32_t>(std::max<size_t>(nb, 1));
  int64_t* d_oidx = A.take<int64_t>(std::max<size_t>(nb, 1));
  double* d_stem = A.take<double>(nb);
  double* d_str = A.take<double>(nb);
  int32_t* d_px = A.take<int32_t>(nb);
  int32_t* d_py = A.take<int32_t>(nb);
  int* d_ctr = A.take<int>(128);  // 16, then kStemQueues item counters per stem class
  int32_t* d_sloty = A.take<int32_t>(std::max<size_t>(plan.slot_y.size(), 1));
  int32_t* d_bx = A.take<int32_t>(std::max<size_t>(plan.big_x.size(), 1));
  int32_t* d_by = A.take<int32_t>(std::max<size_t>(plan.big_x.size(), 1));
  int64_t* d_bo = A.take<int64_t>(std::max<size_t>(plan.big_x.size(), 1));
  int32_t* d_iphi_off = A.take<int32_t>(std::max<size_t>(item_phi_off.size(), 1));
  int32_t* d_iphi = A.take<int32_t>(std::max<size_t>(item_phi.size(), 1));
  int64_t* d_soidx = splan.soidx.empty() ? nullptr : A.take<int64_t>(splan.soidx.size());
  sk::StrPos* d_stab = (splan.n_sfast > splan.n_soh) ? A.take<sk::StrPos>(2 * n_str_pos) : nullptr;
  sk::StrCode* d_ctab = splan.n_soh ? A.take<sk::StrCode>(n_str_pos) : nullptr;

  // parameter tables
  std::vector<double> co(256), st(16);
  const bool subst = kind_subst(kp->kind);
  for (int k = 0; k < 256; ++k)
    co[k] = subst ? std::exp(SK_RIBOSUM_P[k] * kp->beta)
                  : ((k >> 4) == (k & 15) ? kp->stack : kp->covar);
  for (int k = 0; k < 16; ++k)
    st[k] = subst ? std::exp(SK_RIBOSUM_S[k] * kp->alpha)
                  : ((k >> 2) == (k & 3) ? kp->match : kp->mismatch);
  const std::vector<double> gl = gap_powers(kp->loop_gap, max_len + 4);
  const std::vector<double> gs = gap_powers(kp->gap, n_gp_str);
  hipStream_t S = ctx->stream;
  SK_HIP(ctx, sk::h2d(ctx, d_co, co.data(), 256 * 8, S));
  SK_HIP(ctx, sk::h2d(ctx, d_st, st.data(), 16 * 8, S));
  SK_HIP(ctx, sk::h2d(ctx, d_gp_loop, gl.data(), gl.size() * 8, S));
  SK_HIP(ctx, sk::h2d(ctx, d_gp_str, gs.data(), gs.size() * 8, S));
  SK_HIP(ctx, hipMemsetAsync(d_ctr, 0, 128 * sizeof(int), S));

  double* stem_out = (combine_mode(kp->kind) == sk::kCombineStem) ? out_dev : d_stem;
  double* str_out = (combine_mode(kp->kind) == sk::kCombineStr) ? out_dev : d_str;

  // string kernel inputs first: with a stem part it forks to the side stream
  // here, ahead of the stem launches
  const bool side = stem && str;
  if (str) {
    SK_HIP(ctx, sk::h2d(ctx, d_px, splan.spx.empty() ? x : splan.spx.data(), nb * 4, S));
    SK_HIP(ctx, sk::h2d(ctx, d_py, splan.spy.empty() ? y : splan.spy.data(), nb * 4, S));
    if (d_soidx)
      SK_HIP(ctx, sk::h2d(ctx, d_soidx, splan.soidx.data(), splan.soidx.size() * 8, S));
    if (side) {
      SK_HIP(ctx, hipEventRecord(ctx->evf, S));
      SK_HIP(ctx, hipStreamWaitEvent(ctx->side, ctx->evf, 0));
    }
  }
  if (stem) {
    SK_HIP(ctx, sk::h2d(ctx, d_items, plan.items.data(), plan.items.size() * sizeof(int4), S));
    SK_HIP(ctx, sk::h2d(ctx, d_ixs, plan.ixs.data(), nb * 4, S));
    SK_HIP(ctx, sk::h2d(ctx, d_oidx, plan.ioidx.data(), nb * 8, S));
    SK_HIP(ctx, sk::h2d(ctx, d_sloty, plan.slot_y.data(), plan.slot_y.size() * 4, S));
    if (phi_items) {
      SK_HIP(ctx, sk::h2d(ctx, d_iphi_off, item_phi_off.data(), item_phi_off.size() * 4, S));
      if (!item_phi.empty())
        SK_HIP(ctx, sk::h2d(ctx, d_iphi, item_phi.data(), item_phi.size() * 4, S));
    }
    const double gap2 = kp->loop_gap * kp->loop_gap;
    const size_t nnd = std::max<size_t>(PX.nd_a.size(), 1);
    const size_t nxc = std::max<size_t>(PX.xr_ch.size(), 1), nxg = std::max<size_t>(PX.run_rows().size(), 1),
                 nxgc = std::max<size_t>(PX.run_ch().size(), 1),
                 ngh = std::max<size_t>(PX.ex_nl.size() * PX.gam_key.size(), 1),
                 nphk = std::max<size_t>(PX.phk_idx.size(), 1);
    if (!xs_->prep) {
      void* p = nullptr;
      SK_HIP(ctx, hipMalloc(&p, (3 * nnd + nxc + nxg + nxgc + ngh + nphk) * sizeof(double)));
      xs_->prep = static_cast<double*>(p);
      xs_->buf.ptrs.push_back(p);
      xs_->prep_loop_gap = -1.0;
    }
    sk::DevParamNodes pn;
    pn.nd_L = xs_->prep;
    pn.nd_SL = xs_->prep + nnd;
    pn.xr_SL = xs_->prep + 2 * nnd;
    pn.xr_chw = xs_->prep + 3 * nnd;
    pn.xg_SL = pn.xr_chw + nxc;
    pn.xg_chw = pn.xg_SL + nxg;
    pn.gam_h = pn.xg_chw + nxgc;
    pn.phk_w = pn.gam_h + ngh;
    if (!(xs_->prep_loop_gap == kp->loop_gap)) {  // once per dataset and loop_gap
      SK_HIP(ctx, sk::launch_prep(xs_->dev, pn, d_gp_loop, gap2, S));
      xs_->prep_loop_gap = kp->loop_gap;
    }
#ifdef SK_STAMPS
    unsigned long long* d_stamps = nullptr;
    SK_HIP(ctx, hipMalloc(&d_stamps, 16 * sizeof(unsigned long long)));
    SK_HIP(ctx, hipMemsetAsync(d_stamps, 0, 16 * sizeof(unsigned long long), S));
#endif
    if (host_stats)
      std::fprintf(stderr, "[host] pairs=%lld plan %.2f ms, phi keys %.2f ms, uploads+prep %.2f ms\n",
                   (long long)n, th1 - th0, th2 - th1, now_ms() - th2);
    SK_HIP(ctx, hipEventRecord(ctx->ev0, S));
    std::vector<sk::StemLaunch> launches(plan.classes.size());
    for (size_t c = 0; c < plan.classes.size(); ++c) {
      const StemClass& C = plan.classes[c];
      const bool on_cls = two_streams && (c & 1);
      sk::StemLaunch& SL = launches[c];
      SL.xset = xs_->dev;
      SL.yset = ys_->dev;
      SL.pn = pn;
      SL.co_subst = d_co;
      SL.gpow = d_gp_loop;
      SL.n_gpow = max_len + 2;
      SL.n_gpow_pad = (SL.n_gpow + 1) & ~1;
      SL.gap2 = gap2;
      SL.band = kp->len_band;
      SL.lds_max_nl = 64 * C.maxk;
      SL.lds_max_edges = (C.max_edges + 3) & ~3;
      SL.lds_max_bpf = (C.max_bpf + 1 + 3) & ~3;
      SL.lds_max_nch = C.max_nch + 2;  // + 2 dummy chunks read past the end (dag_stem.hip)
      SL.lds_max_len_pad = (max_len + 2 + 3) & ~3;
      SL.items = d_items + C.item_off;
      SL.n_items = (int32_t)C.n_items;
      SL.xs = d_ixs;
      SL.oidx = d_oidx;
      SL.out = stem_out;
      SL.item_counter = d_ctr + 16 + sk::kStemQueues * (int)c;
      for (int q = 0; q <= sk::kStemQueues; ++q) SL.queue_off[q] = C.queue_off[q];
      SL.slab_doubles = (int64_t)(PX.max_slots + 1) * SL.lds_max_nl;
      SL.scratch = on_cls ? scratch_cls : ctx->scratch;
      SL.gam_on = !PX.gam_key.empty();
      SL.gam_doubles = (int64_t)PX.gam_key.size() * SL.lds_max_nl;
      // the workgroups' region: slabs, Gamma tables (unless shared), Phi tables
      double* wg_tab = SL.scratch + (size_t)C.grid * C.nwaves * SL.slab_doubles;
      SL.gam_shared = C.gam_shared ? 1 : 0;
      SL.n_slots = C.gam_shared ? (int32_t)C.n_slots : 0;
      SL.slot_y = d_sloty + C.slot_off;
      SL.gam = C.gam_shared ? scratch_tab + C.tab_off : wg_tab;
      SL.kap_y = SL.gam + C.n_slots * (size_t)SL.gam_doubles;  // (gam_shared: past the class's tables)
      SL.phi_on = phi_on ? 1 : 0;
      SL.phi_shared = C.phi_shared ? 1 : 0;
      SL.phi_doubles = phi_on ? (int64_t)PX.phi_al.size() * (SL.lds_max_nl + 1) : 0;
      // (phi_shared: past the class's Gamma tables and sums)
      SL.phi = C.phi_shared ? SL.kap_y + C.n_slots * PX.gam_key.size()
                            : wg_tab + (C.gam_shared ? 0 : (size_t)C.grid * SL.gam_doubles);
      SL.item_phi_off = d_iphi_off + (phi_items ? C.item_off : 0);
      SL.item_phi = d_iphi;
#ifdef SK_STAMPS
      SL.stamps = d_stamps;
#endif
    }
    // Every class's Gamma tables first (0.2 ms each on a free GPU), ahead of
    // the stem launches of both streams and of the string kernel on the side
    // stream.  A table kernel's workgroups need a stem workgroup's LDS: behind
    // a running persistent launch (another class's, or the string kernel,
    // 50 ms per NS step) they would wait for it to end, and the stem launch
    // behind them with it, instead of filling the GPU as its workgroups retire.
    // The side stream forked at evf, ahead of the stem uploads; waiting for
    // evk as well, its string kernel now also starts behind those uploads
    // (≈ 1 ms per NS step) and, on the first call of a dataset and loop_gap,
    // behind sk_prep_kernel (≈ 20 ms, once).  The table kernels stand outside
    // the class launches' event brackets: sk_last_launch_ms does not count
    // them (0.5 ms per NS step); the stem span (ev0 .. ev1) does.
    bool any_tables = false;
    for (size_t c = 0; c < plan.classes.size(); ++c) {
      SK_HIP(ctx, sk::launch_gamma_tables(launches[c], plan.classes[c].nwaves, S));
      any_tables = any_tables || plan.classes[c].gam_shared;
    }
    if (two_streams || (side && any_tables)) SK_HIP(ctx, hipEventRecord(ctx->evk, S));
    if (two_streams) SK_HIP(ctx, hipStreamWaitEvent(ctx->cls, ctx->evk, 0));
    if (side && any_tables) SK_HIP(ctx, hipStreamWaitEvent(ctx->side, ctx->evk, 0));
    for (size_t c = 0; c < plan.classes.size(); ++c) {
      const StemClass& C = plan.classes[c];
      const bool on_cls = two_streams && (c & 1);
      const sk::StemLaunch& SL = launches[c];
      SK_HIP(ctx, sk::lev_mark(ctx, on_cls ? ctx->cls : S));
      SK_HIP(ctx, sk::launch_stem(SL, C.grid, C.nwaves, on_cls ? ctx->cls : S));
      SK_HIP(ctx, sk::lev_mark(ctx, on_cls ? ctx->cls : S));
      if (C.gam_shared && (C.phi_shared || !phi_on)) ++ctx->last_gamma_shared;
      ctx->last_stem_classes |= 1u << (C.maxk % 4 ? C.maxk : C.maxk / 4);  // (MAXK 17: bit 17)
    }
    if (two_streams) {
      SK_HIP(ctx, hipEventRecord(ctx->evx, ctx->cls));
      SK_HIP(ctx, hipStreamWaitEvent(S, ctx->evx, 0));
    }
    if (!plan.big_x.empty()) {
      const size_t nbig = plan.big_x.size();
      SK_HIP(ctx, sk::h2d(ctx, d_bx, plan.big_x.data(), nbig * 4, S));
      SK_HIP(ctx, sk::h2d(ctx, d_by, plan.big_y.data(), nbig * 4, S));
      SK_HIP(ctx, sk::h2d(ctx, d_bo, plan.big_o.data(), nbig * 8, S));
      sk::StemBigLaunch BL;
      BL.xset = xs_->dev;
      BL.yset = ys_->dev;
      BL.pn = pn;
      BL.co_subst = d_co;
      BL.gpow = d_gp_loop;
      BL.n_gpow = max_len + 2;
      BL.gap2 = gap2;
      BL.band = kp->len_band;
      BL.xs = d_bx;
      BL.ys = d_by;
      BL.oidx = d_bo;
      BL.n_pairs = (int64_t)nbig;
      BL.out = stem_out;
      BL.scratch = ctx->scratch;
      BL.stride = big_stride;
      BL.wave_doubles = big_wave;
      SK_HIP(ctx, sk::lev_mark(ctx, S));
      SK_HIP(ctx, sk::launch_stem_big(BL, big_grid, S));
      SK_HIP(ctx, sk::lev_mark(ctx, S));
      ctx->last_stem_classes |= 1u;
    }
    SK_HIP(ctx, hipEventRecord(ctx->ev1, S));
#ifdef SK_STAMPS
    {
      unsigned long long h[16];
      SK_HIP(ctx, hipMemcpyAsync(h, d_stamps, sizeof(h), hipMemcpyDeviceToHost, S));
      SK_HIP(ctx, hipStreamSynchronize(S));
      (void)hipFree(d_stamps);
      const double rows = (double)h[8];
      std::fprintf(stderr, "[stamps] classes=%zu pairs=%llu rows=%.0f cycles/row:", plan.classes.size(),
                   h[9], rows);
      const char* nm[7] = {"hdr", "A", "Rfill", "passes", "zero", "sweep", "store"};
      for (int i = 0; i < 7; ++i) std::fprintf(stderr, " %s=%.0f", nm[i], h[i] / rows);
      std::fprintf(stderr, "\n[stamps] per row: A-loaded rows=%.3f swept chunks=%.2f match passes=%.2f band nodes=%.1f\n",
                   h[10] / rows, h[11] / rows, h[12] / rows, h[13] / rows);
      for (const StemClass& C : plan.classes)
        std::fprintf(stderr, "[stamps] class maxk=%d max_nl=%d max_edges=%d max_nch=%d waves/wg=%d grid=%d items=%zu\n",
                     C.maxk, C.max_nl, C.max_edges, C.max_nch, C.nwaves, C.grid, C.n_items);
    }
#endif
    ctx->last_launches = (int32_t)plan.classes.size() + (plan.big_x.empty() ? 0 : 1);
  }
  if (str) {
    const hipStream_t SS = side ? ctx->side : S;
    sk::StrLaunch T;
    T.xset = xs_->dev;
    T.yset = ys_->dev;
    T.st = d_st;
    T.gpow = d_gp_str;
    T.gap = kp->gap;
    T.naive = kp->kind == SK_NAIVE_STR ? 1 : 0;
    T.xs = d_px + splan.n_sfast;
    T.ys = d_py + splan.n_sfast;
    T.oidx = d_soidx ? d_soidx + splan.n_sfast : nullptr;
    T.n_pairs = n - splan.n_sfast;
    T.out = str_out;
    T.pair_counter = reinterpret_cast<unsigned long long*>(d_ctr + 8);
    T.lds_max_len = (std::max(PY.max_len, 1) + 1) & ~1;
    // 4 waves per workgroup while their rows fit 64 KB of LDS, fewer for
    // longer y (one wave's rows fit the CU's 160 KB up to L ~ 4,000)
    int w = 4;
    while (w > 1 && sk::str_lds_bytes(T, w) > 65536) w /= 2;
    const size_t lds = sk::str_lds_bytes(T, w);
    if (lds > 163840) return fail(ctx, SK_ERR_UNSUPPORTED, "sequence too long for string kernel LDS");
    const int per_cu = std::max(1, std::min<int>((int)(163840 / lds), 8));
    const int64_t g = std::max<int64_t>(1, std::min<int64_t>((int64_t)ctx->n_cu * per_cu, (n - splan.n_sfast + w - 1) / w));
    SK_HIP(ctx, hipEventRecord(ctx->ev2, SS));
    for (int oh = 1; oh >= 0; --oh) {
      const int64_t b = oh ? 0 : splan.n_soh, e = oh ? splan.n_soh : splan.n_sfast;
      if (e <= b) continue;
      const size_t npx = PX.pos_prof.size(), npy = PY.pos_prof.size();
      const void *tx, *ty;
      if (oh) {  // [npx] x set | [npy] y set
        SK_HIP(ctx, sk::launch_str_code_tab(xs_->dev.pos_prof, xs_->dev.pos_w, (int64_t)npx, d_ctab, SS));
        if (ys_ != xs_)
          SK_HIP(ctx, sk::launch_str_code_tab(ys_->dev.pos_prof, ys_->dev.pos_w, (int64_t)npy, d_ctab + npx, SS));
        tx = d_ctab;
        ty = ys_ != xs_ ? d_ctab + npx : d_ctab;
      } else {   // [npx] x role | [npx] y role (| [npy] x role, unused | [npy] y role)
        SK_HIP(ctx, sk::launch_str_tab(xs_->dev.pos_prof, xs_->dev.pos_w, (int64_t)npx, d_st, d_stab,
                                       d_stab + npx, SS));
        tx = d_stab;
        ty = d_stab + npx;
        if (ys_ != xs_) {
          SK_HIP(ctx, sk::launch_str_tab(ys_->dev.pos_prof, ys_->dev.pos_w, (int64_t)npy, d_st, d_stab + 2 * npx,
                                         d_stab + 2 * npx + npy, SS));
          ty = d_stab + 2 * npx + npy;
        }
      }
      sk::StrFastLaunch F;
      F.xset = xs_->dev;
      F.yset = ys_->dev;
      F.xtab = static_cast<const sk::StrPos*>(tx);
      F.ytab = static_cast<const sk::StrPos*>(ty);
      F.st = d_st;
      F.onehot = oh;
      F.gpow = d_gp_str;
      F.gap = kp->gap;
      F.xs = d_px + b;
      F.ys = d_py + b;
      F.oidx = d_soidx ? d_soidx + b : nullptr;
      F.n_pairs = e - b;
      F.out = str_out;
      F.lds_max_len = (std::max(PY.max_len, 64) + 1) & ~1;
      const size_t wl = sk::str_fast_wave_lds_bytes(F.lds_max_len, oh != 0);
      if (wl + sk::kStrFastLds0 > 163840) return fail(ctx, SK_ERR_UNSUPPORTED, "sequence too long for string kernel LDS");
      const int per_cu_w = (int)std::max<size_t>(1, std::min<size_t>(16, (163840 - sk::kStrFastLds0) / wl));
      const int fw = std::min(4, per_cu_w);
      const int64_t fg = std::min<int64_t>((int64_t)ctx->n_cu * std::max(1, per_cu_w / fw), (e - b + fw - 1) / fw);
      SK_HIP(ctx, sk::launch_str_fast(F, (int)fg, fw, SS));
      ctx->last_str_pairs[oh ? 0 : 1] = e - b;
      ctx->last_str_waves[oh ? 0 : 1] = fw;
    }
    if (splan.n_sfast < n) {
      SK_HIP(ctx, sk::launch_str(T, (int)g, w, SS));
      ctx->last_str_pairs[2] = n - splan.n_sfast;
      ctx->last_str_waves[2] = w;
    }
    SK_HIP(ctx, hipEventRecord(ctx->ev3, SS));
    if (side) {  // join before the combine
      SK_HIP(ctx, hipEventRecord(ctx->evj, ctx->side));
      SK_HIP(ctx, hipStreamWaitEvent(S, ctx->evj, 0));
    }
  }
  const int32_t mode = combine_mode(kp->kind);
  if (mode != sk::kCombineStem && mode != sk::kCombineStr)
    SK_HIP(ctx, sk::launch_combine(d_stem, d_str, out_dev, n, mode, kp->alpha, kp->beta, S));
  // timings: now (synchronous calls), or when sk_sync_timing asks (async)
  SK_HIP(ctx, sk::call_finish(ctx, S, stem, str));
  return SK_OK;
}

}  // namespace sk
