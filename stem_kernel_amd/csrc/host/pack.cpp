// The packer: the host image of a dataset in the layout the kernels read
// (kernels/device_set.h) -- an RNA dataset's x-role and y-role records
// (pack_dataset, in phases: key tables, pack_x per example in pack_x.cpp,
// pack_y per example in pack_y.cpp), a protein dataset's and a palindrome
// dataset's arrays -- and the entry points that upload it or hash it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "host/pack_internal.h"
#include "host/runtime_types.h"

namespace sk {

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

namespace {

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

// SK_PACK_STATS: the row reads the kernel issues for one gamma schedule (its
// rows and child records, each example's first row, row count and first
// record): slab / Gamma / Phi child records, minus the previous row (taken
// from registers); stored rows
struct ScheduleReads {
  long stored = 0, slab = 0, gamma = 0, phi = 0, reg = 0;
};
ScheduleReads schedule_reads(const pvec<XRow>& rows, const pvec<uint32_t>& ch, const std::vector<int32_t>& base,
                             const std::vector<int32_t>& nl, const std::vector<int32_t>& ch_base) {
  ScheduleReads s;
  for (size_t e = 0; e < nl.size(); ++e) {
    uint32_t prev = 0xffffu;
    size_t k = (size_t)ch_base[e];
    for (size_t r = (size_t)base[e]; r < (size_t)base[e] + nl[e]; ++r) {
      const int ne = rows[r].a & 0xff;
      for (int t = 0; t < ne; ++t, ++k) {
        const uint32_t c = ch[k] & 0xffffu;
        if (c == prev) ++s.reg;
        else if (c & 0x8000u) ++s.gamma;
        else if (c & 0x4000u) ++s.phi;
        else ++s.slab;
      }
      prev = rows[r].b >> 16;
      s.stored += prev < 0x4000u;
    }
  }
  return s;
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
namespace {

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// host threads of a packing pass over `jobs` examples (SK_PACK_THREADS caps
// them: the packed arrays do not depend on it, tests/test_pack_threads.py)
int pack_threads(size_t jobs) {
  const size_t pcap = std::getenv("SK_PACK_THREADS") ? (size_t)std::max(1, std::atoi(std::getenv("SK_PACK_THREADS")))
                                                     : (size_t)16;
  return (int)std::max<size_t>(1, std::min<size_t>({jobs / 8 + 1, pcap,
                                                    (size_t)std::max(1u, std::thread::hardware_concurrency())}));
}

// SK_PACK_STATS: rows, unstored rows, slots and row reads of the gamma
// schedule and of the factored one (the one the kernel runs)
void print_schedule_stats(const HostPack& P, long nodes, long unstored, long slots) {
  auto sum = [](const std::vector<int32_t>& v) {
    long s = 0;
    for (int32_t x : v) s += x;
    return s;
  };
  const ScheduleReads g = schedule_reads(P.xgrow, P.xg_ch, P.ex_xg_base, P.ex_nlxg, P.ex_xgch_base);
  fprintf(stderr,
          "[sk pack] gamma schedule: %ld nodes, %ld rows, %ld unstored, %ld slots; stored %ld, reads: "
          "slab %ld gamma %ld phi %ld, from registers %ld\n",
          nodes, sum(P.ex_nlxg), unstored, slots, g.stored, g.slab, g.gamma, g.phi, g.reg);
  if (!P.shared_sums) return;
  const ScheduleReads f = schedule_reads(P.xf_row, P.xf_ch, P.ex_xf_base, P.ex_nlxf, P.ex_xfch_base);
  fprintf(stderr,
          "[sk pack] factored schedule: %ld rows, %ld shared sums for %ld records; stored %ld, reads: "
          "slab %ld gamma %ld phi %ld, from registers %ld\n",
          sum(P.ex_nlxf), sum(P.ex_ss_rows), sum(P.ex_ss_repl), f.stored, f.slab, f.gamma, f.phi, f.reg);
}

// The x role: pack_x per example on host threads, then its arrays appended
// in example order -- the concatenated ones (the *_CAT lists of
// runtime_types.h) at their prefix-sum offsets, copied on the threads.
// yjobs: each example's place in them, for the y role.
int pack_x_role(sk_dataset* ds, const KeyTables& K, double keys_ms, std::vector<YJob>& yjobs, std::string& err) {
  HostPack& P = ds->pack;
  const bool tstats = std::getenv("SK_HOST_STATS") != nullptr;
  const int n = (int)ds->ex.size();
  const int nthr = pack_threads((size_t)n);
  const double tp1 = now_ms();
  std::vector<XOut> xo(n);
  std::atomic<int> next{0};
  auto work = [&]() {
    for (int e = next.fetch_add(1); e < n; e = next.fetch_add(1)) pack_x(ds->ex[e], K, xo[e]);
  };
  run_pool(nthr, work);
  const double tpx = now_ms();
  P.ex_node_base.push_back(0);
  P.ex_edge_base.push_back(0);
  P.ex_bpf_base.push_back(0);
  P.ex_lvl_base.push_back(0);
  P.ex_pos_base.push_back(0);
#define SK_OFF(f) std::vector<size_t> off_##f(n + 1, 0);
  SK_PACK_X_CAT_ARRAYS(SK_OFF)
  SK_PACK_F_CAT_ARRAYS(SK_OFF)
#undef SK_OFF
  auto app = [](auto& dst, const auto& src) { dst.insert(dst.end(), src.begin(), src.end()); };
  long st_nodes = 0, st_nost = 0, st_slots = 0;  // (SK_PACK_STATS)
  yjobs.reserve(n);
  for (int e = 0; e < n; ++e) {
    XOut& O = xo[e];
    if (O.rc) {  // the first failing example, as the serial pass would report it
      err = O.err;
      return O.rc;
    }
    st_nodes += O.n_nodes;
    st_nost += O.n_nostore;
    st_slots += O.gslots;
#define SK_ACC(f) off_##f[e + 1] = off_##f[e] + O.f.size();
    SK_PACK_X_CAT_ARRAYS(SK_ACC)
    SK_PACK_F_CAT_ARRAYS(SK_ACC)
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
  const double tq1 = now_ms();
#define SK_SIZE(f) P.f.resize(off_##f[n]);
  SK_PACK_X_CAT_ARRAYS(SK_SIZE)
  SK_PACK_F_CAT_ARRAYS(SK_SIZE)
#undef SK_SIZE
  const double tq2 = now_ms();
  next = 0;
  auto copy = [&]() {
    for (int e = next.fetch_add(1); e < n; e = next.fetch_add(1)) {
      XOut& O = xo[e];
      for (uint32_t& r : O.gra_row) r += (uint32_t)off_xgrow[e];  // example-local -> dataset row
      for (uint32_t& r : O.xf_gra_row) r += (uint32_t)off_xf_row[e];
#define SK_CPY(f) std::copy(O.f.begin(), O.f.end(), P.f.begin() + off_##f[e]);
      SK_PACK_X_CAT_ARRAYS(SK_CPY)
      SK_PACK_F_CAT_ARRAYS(SK_CPY)
#undef SK_CPY
      O = XOut();  // free as we go
    }
  };
  run_pool(nthr, copy);
  if (tstats) {
    fprintf(stderr, "[sk pack] offsets %.1f ms, resize %.1f ms, copy %.1f ms\n", tq1 - tpx, tq2 - tq1, now_ms() - tq2);
    fprintf(stderr, "[sk pack] keys %.1f ms, x-role %.1f ms (%d threads) + append %.1f ms\n", keys_ms, tpx - tp1, nthr,
            now_ms() - tpx);
  }
  if (std::getenv("SK_PACK_STATS")) print_schedule_stats(P, st_nodes, st_nost, st_slots);
  return SK_OK;
}

// The y role: pack_y per example on host threads over the packed x-role
// arrays, appended like the x role; the renumbered records (r_*) have the
// same sizes at the same offsets.
int pack_y_role(HostPack& P, const std::vector<YJob>& yjobs, std::string& err) {
  const bool tstats = std::getenv("SK_HOST_STATS") != nullptr;
  const double tp2 = now_ms();
  const size_t ny = yjobs.size();
  std::vector<YOut> yo(ny);
  const int nthr = pack_threads(ny);
  std::atomic<size_t> next{0};
  const YOpts yopt = y_opts_from_env();
  SweepCost yc_plain, yc_now;
  long y_renum = 0, mg_plain = 0, mg_now = 0, mg_groups = 0;
  auto work = [&]() {
    for (size_t e = next.fetch_add(1); e < ny; e = next.fetch_add(1)) pack_y(P, yopt, yjobs[e], yo[e]);
  };
  run_pool(nthr, work);
  const double ty1 = now_ms();
#define SK_OFF(f) std::vector<size_t> off_##f(ny + 1, 0);
  SK_PACK_Y_CAT_ARRAYS(SK_OFF)
#undef SK_OFF
  for (size_t e = 0; e < ny; ++e) {
    YOut& Y = yo[e];
    if (!Y.err.empty()) {
      err = Y.err;
      return SK_ERR_INVALID;
    }
#define SK_ACC(f) off_##f[e + 1] = off_##f[e] + Y.f.size();
    SK_PACK_Y_CAT_ARRAYS(SK_ACC)
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
  SK_PACK_Y_CAT_ARRAYS(SK_SIZE)
#undef SK_SIZE
  P.y_renumbered = yopt.renumber;
  if (P.y_renumbered) {
#define SK_SIZE(f) P.r_##f.resize(off_##f[ny]);
    SK_PACK_YREC_ARRAYS(SK_SIZE, )
#undef SK_SIZE
  }
  next = 0;
  auto copy = [&]() {
    for (size_t e = next.fetch_add(1); e < ny; e = next.fetch_add(1)) {
      YOut& Y = yo[e];
#define SK_CPY(f) std::copy(Y.f.begin(), Y.f.end(), P.f.begin() + off_##f[e]);
      SK_PACK_Y_CAT_ARRAYS(SK_CPY)
#undef SK_CPY
      if (P.y_renumbered) {
#define SK_CPY(f) std::copy(Y.r.f.begin(), Y.r.f.end(), P.r_##f.begin() + off_##f[e]);
        SK_PACK_YREC_ARRAYS(SK_CPY, )
#undef SK_CPY
      }
      Y = YOut();  // free as we go
    }
  };
  run_pool(nthr, copy);
  long tch = 0;
  for (int32_t c : P.ex_nch) tch += c;
  if (tstats)
    fprintf(stderr, "[sk pack] y-role %.1f ms (%d threads) + append %.1f ms; sweep chunks %ld (%.2f per y)\n",
            ty1 - tp2, nthr, now_ms() - ty1, tch, P.ex_nch.empty() ? 0.0 : (double)tch / P.ex_nch.size());
  if (yopt.stats) {  // the sweep's and the MATCH gather's bank model, plain order by length and as packed
    const double d = (double)std::max(tch, 1l), g = (double)std::max(mg_groups, 1l);
    fprintf(stderr,
            "[sk pack] sweep bank model over %ld chunks: plain order read %.3f atomic %.3f cycles per chunk, "
            "packed read %.3f atomic %.3f (%ld of %zu y renumbered); MATCH gather read cycles per 64-edge "
            "group: plain %.3f packed %.3f\n",
            tch, yc_plain.read / d, yc_plain.atomic / d, yc_now.read / d, yc_now.atomic / d, y_renum, ny,
            mg_plain / g, mg_now / g);
  }
  return SK_OK;
}

}  // namespace

int pack_dataset(sk_dataset* ds, std::string& err, const std::function<void()>* after_x) {
  HostPack& P = ds->pack;
  const double tp0 = now_ms();
  P = HostPack();
  const KeyTables K = key_tables(ds->ex, pack_threads(ds->ex.size()));
  P.gam_key = K.gam_key;
  P.shared_sums = K.ss_on;
  if (K.phi_on)
    for (uint64_t k : K.phi_raw) {
      P.phi_al.push_back((uint32_t)k);
      P.phi_g.push_back(K.gamma_idx((uint32_t)(k >> 32)));
    }
  std::vector<YJob> yjobs;
  if (const int rc = pack_x_role(ds, K, now_ms() - tp0, yjobs, err)) return rc;
  // the x-role arrays are final: the caller may start uploading them while
  // the y-role records are formed (sk_dataset_upload)
  if (after_x) (*after_x)();
  return pack_y_role(P, yjobs, err);
}

// ---------------------------------------------------------------- uploads
namespace {

// a palindrome dataset has its own image (sk::SimpalSet)
int upload_palindromes(sk_context* ctx, sk_dataset* ds) {
  size_t m = 0;
  for (const Example& X : ds->ex) m += X.pal_key.size();
  if (m > (size_t)INT32_MAX) return fail(ctx, SK_ERR_UNSUPPORTED, "palindrome dataset too large");
  try {
    pack_palindromes(ds);
  } catch (const std::bad_alloc&) {
    return fail(ctx, SK_ERR_ALLOC, "palindrome pack");
  }
  const sk_dataset::PalPack& Q = ds->spack;
  SK_HIP(ctx, upload(ds->buf, Q.ex_off, &ds->sdev.ex_off));
  SK_HIP(ctx, upload(ds->buf, Q.key, &ds->sdev.key));
  SK_HIP(ctx, upload(ds->buf, Q.dist, &ds->sdev.dist));
  SK_HIP(ctx, upload(ds->buf, Q.w, &ds->sdev.w));
  ds->spack.key = std::vector<uint64_t>();  // (the device holds them; the host plan reads the offsets)
  ds->spack.dist = std::vector<int32_t>();
  ds->spack.w = std::vector<float>();
  ds->device = ctx->device;
  ds->uploaded = true;
  return SK_OK;
}

// a protein dataset has its own image (sk::LaProtSet)
int upload_protein(sk_context* ctx, sk_dataset* ds) {
  size_t pos = 0;
  for (const Example& X : ds->ex) pos += (size_t)X.len;
  if (pos > (size_t)INT32_MAX) return fail(ctx, SK_ERR_UNSUPPORTED, "protein dataset too large");
  try {
    pack_protein(ds);
  } catch (const std::bad_alloc&) {
    return fail(ctx, SK_ERR_ALLOC, "protein pack");
  }
  const sk_dataset::ProtPack& Q = ds->ppack;
  SK_HIP(ctx, upload(ds->buf, Q.ex_len, &ds->pdev.ex_len));
  SK_HIP(ctx, upload(ds->buf, Q.ex_pos_base, &ds->pdev.ex_pos_base));
  SK_HIP(ctx, upload(ds->buf, Q.prof, &ds->pdev.prof));
  SK_HIP(ctx, upload(ds->buf, Q.code, &ds->pdev.code));
  ds->ppack.prof = std::vector<float>();  // (the device holds them; the host plan reads lengths and flags)
  ds->ppack.code = std::vector<uint8_t>();
  ds->device = ctx->device;
  ds->uploaded = true;
  return SK_OK;
}

// the x-role arrays of P to the device image D (on the calling thread, which
// may be a second one: it sets the device itself)
hipError_t upload_x_role(int device, DeviceBuffers& B, const HostPack& P, DevSet& D) {
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return e;
#define SK_UPX(f, d) \
  if ((e = upload(B, P.f, &D.d)) != hipSuccess) return e;
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
    if ((e = upload(B, grb, &D.ex_gr_base)) != hipSuccess) return e;
    std::vector<int32_t> b1 = P.ex_gra_base, b2 = P.ex_phk_base;
    b1.push_back((int32_t)P.gra_gidx.size());
    b2.push_back((int32_t)P.phk_idx.size());
    if ((e = upload(B, b1, &D.ex_gra_base)) != hipSuccess) return e;
    if ((e = upload(B, b2, &D.ex_phk_base)) != hipSuccess) return e;
  }
#undef SK_UPX
  return hipSuccess;
}

}  // namespace

}  // namespace sk

extern "C" {

int sk_dataset_upload(sk_context* ctx, sk_dataset* ds) {
  if (!ctx || !ds) return SK_ERR_INVALID;
  if (ds->uploaded) return ds->device == ctx->device ? SK_OK : sk::fail(ctx, SK_ERR_INVALID, "dataset bound to another device");
  SK_HIP(ctx, hipSetDevice(ctx->device));
  if (sk::ds_pal(ds)) return sk::upload_palindromes(ctx, ds);
  if (sk::ds_protein(ds)) return sk::upload_protein(ctx, ds);
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
  const std::function<void()> after_x = [&]() {
    P.xr_ch.insert(P.xr_ch.end(), 8, 0u);  // the kernel prefetches 4 records past a row
    P.xg_ch.insert(P.xg_ch.end(), 8, 0u);
    if (P.shared_sums) P.xf_ch.insert(P.xf_ch.end(), 8, 0u);
    auto job = [&]() {
      const auto t0 = std::chrono::steady_clock::now();
      xe = sk::upload_x_role(ctx->device, B, P, D);
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
    sk::YOpts opt = sk::y_opts_from_env();
    opt.renumber = opt.renumber && !plain;
    opt.stats = false;
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
