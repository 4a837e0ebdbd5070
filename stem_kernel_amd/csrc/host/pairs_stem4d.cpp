// Planner of the 4-D stem kernel (kernels/stem4d.hip, kernels/phmm.hip): the
// dataset's resident tables, the batches and their span and column launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "host/runtime_types.h"

namespace sk {
namespace {

// 4-D stem kernel: per example, the lowercased sequence (the loader's
// ToLower, common/example.cpp:26-34) and BPMat::prob(a, b) for a <= b by
// diagonal e = b - a (prob(a,a) = 0), as float (stem_kernel.cpp:320, 328).
void stem4d_tables(const Example& X, const sk_kernel_params* kp, std::vector<float>& bp,
                   std::vector<uint8_t>& chr) {
  const int L = X.len;
  std::string s = X.rows[0];
  for (char& c : s) c = (char)std::tolower((unsigned char)c);
  chr.assign(s.begin(), s.end());
  chr.push_back(0);
  bp.clear();
  for (int e = 0; e < L; ++e)
    for (int a = 0; a + e < L; ++a) {
      const int b = a + e;
      float v = 0.0f;
      if (kp->bp_model == 0) {
        if (e > 0) v = (float)X.bpp[sk::tri_index(L, a, b)];
      } else {  // NormalBasePair / WobbleBasePair (stem_kernel.cpp:354-396)
        const char p = s[a], q = s[b];
        bool ok = (p == 'a' && q == 'u') || (p == 'u' && q == 'a') || (p == 'g' && q == 'c') ||
                  (p == 'c' && q == 'g');
        if (kp->bp_model == 2) ok = ok || (p == 'g' && q == 'u') || (p == 'u' && q == 'g');
        v = ((unsigned)a + 1 + kp->loop <= (unsigned)b && ok) ? 1.0f : 0.0f;
      }
      bp.push_back(v);
    }
}

static int stem4d_dataset_tables(sk_context* ctx, sk_dataset* ds, const sk_kernel_params* kp,
                                 std::shared_ptr<const Stem4dTables>* out) {
  std::lock_guard<std::mutex> lk(ds->s4_mu);
  auto same = [&](const std::shared_ptr<Stem4dTables>& t) {
    return t->device == ctx->device && t->model == kp->bp_model && t->loop == kp->loop;
  };
  auto it = std::find_if(ds->s4.begin(), ds->s4.end(), same);
  if (it != ds->s4.end() && (*it)->n_ex == ds->ex.size()) {
    *out = *it;
    return SK_OK;
  }
  auto tp = std::make_shared<Stem4dTables>();
  Stem4dTables& T = *tp;
  const size_t n = ds->ex.size();
  std::vector<float> bpall, bp;
  std::vector<uint8_t> chall, chr;
  T.bp_off.assign(n, -1);
  T.ch_off.assign(n, -1);
  T.why.assign(n, 0);
  T.acgu.assign(n, 0);
  for (size_t e = 0; e < n; ++e) {
    const Example& X = ds->ex[e];
    if (X.n_rows != 1) {
      T.why[e] = 1;
      continue;
    }
    if (kp->bp_model == 0 && !X.has_bp) {
      T.why[e] = 2;
      continue;
    }
    stem4d_tables(X, kp, bp, chr);
    T.acgu[e] = 1;
    for (int a = 0; a < X.len; ++a)
      if (!std::strchr("acgu", (char)chr[a]) || !chr[a]) T.acgu[e] = 0;
    T.bp_off[e] = (int64_t)bpall.size();
    T.ch_off[e] = (int64_t)chall.size();
    bpall.insert(bpall.end(), bp.begin(), bp.end());
    chall.insert(chall.end(), chr.begin(), chr.end());
  }
  T.device = ctx->device;
  SK_HIP(ctx, upload(T.buf, bpall, &T.bp));
  SK_HIP(ctx, upload(T.buf, chall, &T.ch));
  T.model = kp->bp_model;
  T.loop = kp->loop;
  T.n_ex = n;
  // the set it replaces is freed once no call holds it (after its device
  // synchronizes, ~Stem4dTables)
  if (it != ds->s4.end()) {
    *it = tp;
  } else {
    if (ds->s4.size() >= kS4Sets) ds->s4.erase(ds->s4.begin());
    ds->s4.push_back(tp);
  }
  *out = tp;
  return SK_OK;
}

int64_t stem4d_plane_doubles(int m) {
  int64_t r = 0;
  for (int d2 = 0; d2 <= m; ++d2) r += ((m + 1 - d2) + 3) & ~3;
  return r;
}

// waves per pair of the column kernel for a batch whose y lengths lie in
// [min_m, max_m] (min_m counts |y| >= 2 only; INT32_MAX for none)
static int col_waves(int cpl, int min_m, int max_m, int max_n) {
  static const int w_env = SK_KNOB("SK4C_W") ? std::max(1, std::atoi(SK_KNOB("SK4C_W"))) : 0;
  int W = std::min(w_env ? w_env : sk::stem4d_col_max_waves(cpl), sk::stem4d_col_max_waves(cpl));
  if (min_m != INT32_MAX) W = std::min(W, sk::stem4d_col_w_max(min_m));
  W = std::max(W, 1);
  while (W > 1 && sk::stem4d_col_lds_bytes(cpl, W, max_m, max_n) > 160 * 1024) --W;
  return W;
}

}  // namespace

int run_stem4d(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
               const int32_t* x, const int32_t* y, int64_t n, double* out_dev) {
  if (kp->bp_model < 0 || kp->bp_model > 2 || !(kp->bp_bound >= 0.0))
    return fail(ctx, SK_ERR_INVALID, "4-D stem kernel: bp_model 0..2 and bp_bound >= 0");
  // StemKernel::operator() (stem_kernel.h:52-55): partial_dp when ali_bound
  // > 0 or band > 0; ali_bound is a float option
  const float ali_bound = (float)kp->ali_bound;
  const bool ali = ali_bound > 0.0f;  // -a: residues must be ACGU
  // Anchors come from the PairHMM only with the intended zerop.  As the
  // reference builds today (ali_zerop_fixed 0) every posterior is NaN, no
  // position is anchored and the constraints are [0, |y|] for every x
  // position whatever the band (checked against the oracle's
  // full NaN-propagating restatement), and partial_dp over the full range is
  // full_dp operation for operation.
  const bool ali_phmm = ali && kp->ali_zerop_fixed;
  // per-example tables, resident per dataset (built on first use)
  std::shared_ptr<const Stem4dTables> tx, ty;
  int rc = stem4d_dataset_tables(ctx, xs_, kp, &tx);
  if (rc) return rc;
  if (ys_ == xs_) ty = tx;
  else if ((rc = stem4d_dataset_tables(ctx, ys_, kp, &ty))) return rc;
  const Stem4dTables& TX = *tx;
  const Stem4dTables& TY = *ty;
  auto usable = [&](const Stem4dTables& T, int e) -> int {
    if (T.why[e] == 1) return fail(ctx, SK_ERR_INVALID, "4-D stem kernel takes single sequences");
    if (T.why[e] == 2) return fail(ctx, SK_ERR_INVALID, "4-D stem kernel with bp_model 0 needs base pairs");
    if (ali && !T.acgu[e])  // PairHMM's char2rna asserts on anything else (phmm.cpp:247-258)
      return fail(ctx, SK_ERR_INVALID, "4-D stem kernel: alignment constraints need A/C/G/U sequences");
    return SK_OK;
  };
  int max_m = 0, max_n = 0;
  double cells = 0.0;
  for (int64_t k = 0; k < n; ++k) {
    if ((rc = usable(TX, x[k])) || (rc = usable(TY, y[k]))) return rc;
    const double a = xs_->ex[x[k]].len, b = ys_->ex[y[k]].len;
    max_m = std::max(max_m, (int)b);
    max_n = std::max(max_n, (int)a);
    cells += (a + 1) * (a + 2) / 2 * (b + 1) * (b + 2) / 2;
  }
  ctx->last_cells = cells;
  // batches bounded by scratch memory
  size_t free_b = 0, total_b = 0;
  SK_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
  const double budget = std::min(128e9, 0.5 * (double)free_b);
  std::vector<int64_t> order(n);
  std::iota(order.begin(), order.end(), 0);
  // g^k for y spans (d1 = 0 planes) and, in the column kernel, x spans (the
  // diagonal cells G0(i, j, l, l) = g^(j-i))
  const std::vector<double> gp = gap_powers(kp->gap, std::max(max_m, max_n) + 2);
  rc = ensure_work(ctx, gp.size() * 8 + 4096);
  if (rc) return rc;
  Arena A{static_cast<char*>(ctx->work), 0, ctx->work_bytes};
  double* d_gp = A.take<double>(gp.size());
  hipStream_t S = ctx->stream;
  SK_HIP(ctx, hipMemcpyAsync(d_gp, gp.data(), gp.size() * 8, hipMemcpyHostToDevice, S));
  const int cpl = sk::stem4d_cpl(max_m);
  // |y| >= 512: the kernel sweeps k tiles of 512 and hands each tile's first
  // K3/G3 column to the next through per-item boundary columns
  const bool ktiles = max_m + 1 > 64 * cpl;
  const int64_t kb_stride = ktiles ? 4 * (int64_t)(max_m + 1) : 0;
  // full_dp: G-only planes with the K chain summed (stem4d.hip); the banded
  // and PairHMM-constrained partial_dp keep the four-state planes (their
  // boundary approximations read K0 / K1 off the band)
  const bool banded = ali_phmm || (!ali && kp->len_band > 0);
  const bool gsum = !banded && !SK_KNOB("SK4_NO_GSUM");
  const size_t nst = gsum ? 2 : 4;
  // full_dp with one k tile: the column-group kernel (one workgroup per pair,
  // B' handed on through LDS, NB columns chained per position;
  // stem4d.hip sk_stem4d_col_kernel); SK4_SPAN=1 (per call, A/B) runs the
  // pre-combined span kernel instead, SK4_NO_PRE=1 the K-sum span kernel
  // (pairs whose y is too short for the column schedule, 2 <= m < 2 PF + 3,
  // go to the span kernel in batches of their own)
  const bool colk_call = gsum && !ktiles && !SK_KNOB("SK4_SPAN") && !SK_KNOB("SK4_NO_PRE");
  const int col_nb = colk_call ? sk::stem4d_col_nb(cpl) : 0;
  // (|x| <= stem4d_col_max_n(): the kernel holds x in LDS and counts its
  // steps in an int; longer x take the span kernel)
  auto col_ok = [&](int64_t q) {
    const int m = ys_->ex[y[q]].len;
    return colk_call && xs_->ex[x[q]].len <= sk::stem4d_col_max_n() &&
           (m <= 1 || sk::stem4d_col_w_max(m) >= 1);
  };
  // batches of one kernel: the column kernel's pairs first, then longest x first
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
    const bool ca = col_ok(a), cb = col_ok(b);
    if (ca != cb) return ca;
    return xs_->ex[x[a]].len > xs_->ex[x[b]].len;
  });
  double total_ms = 0.0;
  int launches = 0;
  Stem4dBatch& Bt = ctx->s4d;
  for (int64_t b0 = 0; b0 < n;) {
    // pairs of this batch and their scratch
    std::vector<sk::Stem4dPair> prs;
    double bytes = 0.0;     // rings + boundary columns (the budget)
    size_t ring_bytes = 0;  // rings only: pair p's at scratch_off, boundary columns after all
    int64_t b1 = b0;
    int maxn = 0;
    const bool colk = col_ok(order[b0]);
    while (b1 < n && prs.size() < 4096 && col_ok(order[b1]) == colk) {
      const int64_t q = order[b1];
      sk::Stem4dPair p;
      p.n = xs_->ex[x[q]].len;
      p.m = ys_->ex[y[q]].len;
      p.plane_doubles = stem4d_plane_doubles(p.m);
      // column kernel: n G0 planes (slot i) + the round wrap's NB B' planes;
      // span kernels: a ring of three spans of n + 1 planes (+ acc)
      const size_t rb = colk ? ((size_t)(p.n + col_nb) * (size_t)p.plane_doubles * 8 + 255) & ~(size_t)255
                             : ((size_t)3 * (p.n + 1) * nst * (size_t)p.plane_doubles * 8 +
                                (gsum ? (size_t)(p.n + 1) * 8 : 0) + 255) & ~(size_t)255;
      const double pb = (double)rb + (double)(p.n + 1) * (double)kb_stride * 8.0;
      if (!prs.empty() && bytes + pb > budget) break;
      p.scratch_off = (int64_t)(ring_bytes / 8);
      bytes += pb;
      ring_bytes += rb;
      p.x_bp = TX.bp_off[x[q]];
      p.x_chr = TX.ch_off[x[q]];
      p.y_bp = TY.bp_off[y[q]];
      p.y_chr = TY.ch_off[y[q]];
      p.out_index = q;
      maxn = std::max(maxn, p.n);
      prs.push_back(p);
      ++b1;
    }
    if (colk) {
      // one launch for the batch: W waves per pair, W <= m - 2 PF - 2 for
      // every pair (the round wrap's lag, stem4d.hip kS4cV; |y| <= 1: no
      // stacking source, K = 1 without a step), the class's register budget
      // and 160 KB of LDS (SK4C_W: fewer, A/B)
      int min_m = INT32_MAX;
      for (const auto& p : prs)
        if (p.m >= 2) min_m = std::min(min_m, p.m);
      const int W = col_waves(cpl, min_m, max_m, maxn);
      rc = ensure_scratch(ctx, ring_bytes + 64);
      if (rc) return rc;
      if (Bt.cap_pairs < prs.size()) {
        if (Bt.pairs) {
          SK_HIP(ctx, hipStreamSynchronize(S));
          (void)hipFree(Bt.pairs);
        }
        Bt.cap_pairs = std::max<size_t>(prs.size(), 64);
        SK_HIP(ctx, hipMalloc(&Bt.pairs, Bt.cap_pairs * sizeof(sk::Stem4dPair)));
      }
      SK_HIP(ctx, hipMemcpyAsync(Bt.pairs, prs.data(), prs.size() * sizeof(sk::Stem4dPair),
                                 hipMemcpyHostToDevice, S));
      sk::Stem4dLaunch L;
      L.pairs = Bt.pairs;
      L.scratch = ctx->scratch;
      L.bpdiag = TX.bp;
      L.chars = TX.ch;
      L.bpdiag_y = TY.bp;
      L.chars_y = TY.ch;
      L.gpow = d_gp;
      L.gap = kp->gap;
      L.stack = kp->stack;
      L.subst = kp->subst;
      L.bp_bound = (float)kp->bp_bound;
      L.out = out_dev;
      L.gsum = 3;
      SK_HIP(ctx, hipEventRecord(ctx->ev0, S));
      SK_HIP(ctx, sk::lev_mark(ctx, S));
      SK_HIP(ctx, sk::launch_stem4d_col(L, (int64_t)prs.size(), cpl, W, max_m, maxn, S));
      SK_HIP(ctx, sk::lev_mark(ctx, S));
      ctx->last_s4d_classes |= 1u << ((cpl == 1 ? 0 : cpl == 2 ? 1 : cpl == 4 ? 2 : 3) + 8);
      ++launches;
      SK_HIP(ctx, hipEventRecord(ctx->ev1, S));
      SK_HIP(ctx, hipStreamSynchronize(S));
      SK_HIP(ctx, sk::lev_collect(ctx));
      float ms = 0.f;
      SK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
      total_ms += ms;
      b0 = b1;
      continue;
    }
    // partial_dp constraints per pair: x position -> [c_low, c_high].  With
    // -a the PairHMM kernel writes them on the device; with -b alone
    // (alignment_constraints with ali_bound 0, stem_kernel.cpp:68-74) they
    // are formed here.
    std::vector<int32_t> blo, bhi;
    size_t n_band = 0;
    int max_n1 = 1, max_m1 = 1;
    if (ali_phmm) {
      for (auto& p : prs) {
        p.band_off = (int64_t)n_band;
        n_band += (size_t)p.n + 1;
        max_n1 = std::max(max_n1, p.n + 1);
        max_m1 = std::max(max_m1, p.m + 1);
      }
    } else if (!ali && kp->len_band > 0) {
      for (auto& p : prs) {
        p.band_off = (int64_t)blo.size();
        for (int i = 0; i <= p.n; ++i) {
          const unsigned jj = p.n ? (unsigned)((double)i / p.n * p.m + 0.5) : 0u;
          blo.push_back((int32_t)(jj < kp->len_band ? 0u : jj - kp->len_band));
          bhi.push_back((int32_t)(jj + kp->len_band > (unsigned)p.m ? (unsigned)p.m : jj + kp->len_band));
        }
      }
    }
    // work items {pair, i} per span d1 and part, concatenated: the pairs are
    // dealt to nh parts whose launches run on their own streams (main, class,
    // side, aux), so each span's tail overlaps the other parts' launches (the
    // boundary columns of k tiles are per launch item: one stream then)
    int nh = SK_KNOB("SK4_STREAMS") ? std::atoi(SK_KNOB("SK4_STREAMS")) : 4;
    if (SK_KNOB("SK_SERIAL_CLASSES") || ktiles) nh = 1;
    nh = std::max(1, std::min({nh, 4, (int)prs.size()}));
    const hipStream_t hs[4] = {S, ctx->cls, ctx->side, ctx->aux};
    std::vector<int2> items;
    std::vector<int64_t> ioff((size_t)(maxn + 1) * nh + 1, 0);
    for (int d1 = 0; d1 <= maxn; ++d1)
      for (int h = 0; h < nh; ++h) {
        ioff[(size_t)d1 * nh + h] = (int64_t)items.size();
        for (size_t p = h; p < prs.size(); p += nh)
          for (int i = 0; i + d1 <= prs[p].n; ++i) items.push_back(make_int2((int)p, i));
      }
    ioff.back() = (int64_t)items.size();
    if (!ali_phmm) n_band = blo.size();
    const size_t phmm_bytes =
        ali_phmm ? prs.size() * sk::phmm_pair_bytes(max_n1, max_m1) : 0;
    // boundary columns after the rings: at most the d1 = 0 launch's items
    const size_t kb_bytes = ktiles ? (size_t)(ioff[nh] - ioff[0]) * (size_t)kb_stride * 8 : 0;
    rc = ensure_scratch(ctx, std::max(ring_bytes + kb_bytes + 64, phmm_bytes));
    if (rc) return rc;
    if (Bt.cap_pairs < prs.size() || Bt.cap_items < items.size()) {
      if (Bt.pairs) (void)hipFree(Bt.pairs);
      if (Bt.items) (void)hipFree(Bt.items);
      Bt.cap_pairs = std::max<size_t>(prs.size(), 64);
      Bt.cap_items = std::max<size_t>(items.size(), 4096);
      SK_HIP(ctx, hipMalloc(&Bt.pairs, Bt.cap_pairs * sizeof(sk::Stem4dPair)));
      SK_HIP(ctx, hipMalloc(&Bt.items, Bt.cap_items * sizeof(int2)));
    }
    SK_HIP(ctx, hipMemcpyAsync(Bt.pairs, prs.data(), prs.size() * sizeof(sk::Stem4dPair),
                               hipMemcpyHostToDevice, S));
    SK_HIP(ctx, hipMemcpyAsync(Bt.items, items.data(), items.size() * sizeof(int2),
                               hipMemcpyHostToDevice, S));
    if (n_band) {
      if (Bt.cap_band < n_band) {
        if (Bt.band) {
          SK_HIP(ctx, hipStreamSynchronize(S));
          (void)hipFree(Bt.band);
        }
        Bt.cap_band = std::max<size_t>(n_band, 4096);
        SK_HIP(ctx, hipMalloc(&Bt.band, 2 * Bt.cap_band * sizeof(int32_t)));
      }
      if (!blo.empty()) {
        SK_HIP(ctx, hipMemcpyAsync(Bt.band, blo.data(), blo.size() * 4, hipMemcpyHostToDevice, S));
        SK_HIP(ctx, hipMemcpyAsync(Bt.band + Bt.cap_band, bhi.data(), bhi.size() * 4,
                                   hipMemcpyHostToDevice, S));
      }
    }
    sk::Stem4dLaunch L;
    L.pairs = Bt.pairs;
    L.scratch = ctx->scratch;
    L.bpdiag = TX.bp;
    L.chars = TX.ch;
    L.bpdiag_y = TY.bp;
    L.chars_y = TY.ch;
    L.gpow = d_gp;
    L.gap = kp->gap;
    L.stack = kp->stack;
    L.subst = kp->subst;
    L.bp_bound = (float)kp->bp_bound;
    L.out = out_dev;
    L.band_lo = n_band ? Bt.band : nullptr;
    L.band_hi = n_band ? Bt.band + Bt.cap_band : nullptr;
    L.kbound = ktiles ? ctx->scratch + ring_bytes / 8 : nullptr;
    L.kbound_stride = kb_stride;
    // one k tile: each plane's stacking chain produced one span early by the
    // plane that streams its G0 rows (stem4d.hip sk_stem4d_pre_kernel)
    const bool no_pre = SK_KNOB("SK4_NO_PRE") != nullptr;  // per call (A/B tests)
    L.gsum = gsum ? (!ktiles && !no_pre ? 2 : 1) : 0;
    SK_HIP(ctx, hipEventRecord(ctx->ev0, S));
    if (ali_phmm) {
      sk::PhmmLaunch H;
      H.pairs = Bt.pairs;
      H.n_pairs = (int64_t)prs.size();
      H.chars = TX.ch;
      H.chars_y = TY.ch;
      H.scratch = reinterpret_cast<char*>(ctx->scratch);
      H.n1 = max_n1;
      H.m1 = max_m1;
      H.pair_bytes = sk::phmm_pair_bytes(max_n1, max_m1);
      H.ali_bound = ali_bound;
      H.band = kp->len_band;
      H.zerop_fixed = kp->ali_zerop_fixed ? 1 : 0;
      H.band_lo = Bt.band;
      H.band_hi = Bt.band + Bt.cap_band;
      SK_HIP(ctx, sk::launch_phmm(H, S));
    }
    if (nh > 1) {
      SK_HIP(ctx, hipEventRecord(ctx->evk, S));
      for (int h = 1; h < nh; ++h) SK_HIP(ctx, hipStreamWaitEvent(hs[h], ctx->evk, 0));
    }
    for (int d1 = 0; d1 <= maxn; ++d1)
      for (int h = 0; h < nh; ++h) {
        const size_t q = (size_t)d1 * nh + h;
        L.d1 = d1;
        L.items = Bt.items + ioff[q];
        L.n_items = ioff[q + 1] - ioff[q];
        if (!L.n_items) continue;
        SK_HIP(ctx, sk::lev_mark(ctx, hs[h]));
        SK_HIP(ctx, sk::launch_stem4d(L, cpl, hs[h]));
        SK_HIP(ctx, sk::lev_mark(ctx, hs[h]));
        ctx->last_s4d_classes |= 1u << ((cpl == 1 ? 0 : cpl == 2 ? 1 : cpl == 4 ? 2 : 3) +
                                        (L.band_lo ? 4 : 0));
        ++launches;
      }
    for (int h = 1; h < nh; ++h) {
      hipEvent_t e = h == 1 ? ctx->evx : h == 2 ? ctx->evj : ctx->eva;
      SK_HIP(ctx, hipEventRecord(e, hs[h]));
      SK_HIP(ctx, hipStreamWaitEvent(S, e, 0));
    }
    SK_HIP(ctx, hipEventRecord(ctx->ev1, S));
    SK_HIP(ctx, hipStreamSynchronize(S));
    SK_HIP(ctx, sk::lev_collect(ctx));
    float ms = 0.f;
    SK_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    total_ms += ms;
    b0 = b1;
  }
  ctx->last_stem_ms = total_ms;
  ctx->last_launches = launches;
  return SK_OK;
}

}  // namespace sk

extern "C" {

int sk_stem4d_col_shape(int32_t min_len, int32_t max_len, int32_t* nb, int32_t* waves, int32_t* pf) {
  if (max_len < 0 || min_len > max_len) return SK_ERR_INVALID;
  const int cpl = sk::stem4d_cpl(max_len);
  // the shape of the launch that actually runs (a Gram: x and y lengths in
  // [min_len, max_len]); waves = 0 where the column kernel does not run --
  // |y| >= 512 (k tiles), |x| past its LDS / step-count limit, or a y too
  // short for the column schedule (those pairs take the span kernel)
  const bool runs = max_len + 1 <= 64 * cpl && max_len <= sk::stem4d_col_max_n() &&
                    (min_len <= 1 || sk::stem4d_col_w_max(min_len) >= 1);
  if (nb) *nb = sk::stem4d_col_nb(cpl);
  if (waves) *waves = runs ? sk::col_waves(cpl, min_len >= 2 ? min_len : INT32_MAX, max_len, max_len) : 0;
  if (pf) *pf = sk::stem4d_col_pf();
  return SK_OK;
}

}  // extern "C"
