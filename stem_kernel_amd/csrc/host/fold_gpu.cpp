// The GPU folds: the McCaskill fold, structure sampling and the consensus fold
// of alignments go through one batch driver (fold_batches; host pieces:
// host/fold_host.cpp), and the dataset adders that fold their examples first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "host/fold_host.h"
#include "host/runtime_types.h"
#include "kernels/fold_ali_model.h"
#include "kernels/fold_rng.h"

namespace sk {
namespace {

// What the single-sequence fold and the consensus fold give the driver
struct FoldKind {
  int tables;                                              // n x n work tables per item
  double (*more_bytes)(double n, double rows, bool no_lp);  // an item's share of the memory budget besides them
  void (*lonely)(const int8_t* c, int n_rows, int n, bool no_gu, uint8_t* lp);  // --noLonelyPairs filter of an item
  void (*more_tables)(sk::FoldLaunch&, std::vector<double>&);                   // after fold_tables (nullptr: none)
  sk::FoldPath (*path)(const sk::FoldLaunch&, int);  // the kernel a launch runs (lds_bytes and launch go by it)
  size_t (*lds_bytes)(const sk::FoldLaunch&, int);
  hipError_t (*launch)(const sk::FoldLaunch&, int, int, hipStream_t);
  const char *too_long, *out_of_range;  // the wording of its errors
};
const FoldKind kFoldPlain = {
    sk::kFoldTables, [](double, double, bool) { return 0.0; },
    [](const int8_t* c, int, int n, bool no_gu, uint8_t* lp) { sk::lonely_pair_table(c, n, no_gu, lp); }, nullptr,
    sk::fold_path, sk::fold_lds_bytes, sk::launch_fold, "fold: sequence too long for the fold kernel's LDS",
    "fold: partition function out of double range (sequence too long)"};
const FoldKind kFoldAli = {
    sk::kFoldAliTables, [](double n, double rows, bool no_lp) { return n * rows + (no_lp ? n * n : 0.0); },
    sk::lonely_pair_table_ali, sk::fold_tables_ali, sk::fold_ali_path, sk::fold_ali_lds_bytes,
    sk::launch_fold_ali,
    "consensus fold: alignment too long for the kernel's LDS",
    "consensus fold: partition function out of double range (alignment too long)"};

// what sk_fold_sample adds to a fold call: after the inside pass of each
// batch, n_samples structures per sequence are drawn on the same stream
struct FoldSampling {
  int32_t n_samples = 0;
  uint64_t seed = 0;
  char* structs = nullptr;  // optional, sk_fold_sample's out_structs
};

// n items, item k of n_rows[k] rows (nullptr: one each) of equal length, the
// items' rows back to back in rows, in batches whose tables fit the memory
// budget: out gets the probabilities (sm: optional, count / n_samples)
int fold_batches(sk_context* ctx, const FoldKind& K, int32_t n, const int32_t* n_rows, const char* const* rows,
                 int32_t flags, double* out, double* log_z, const FoldSampling* sm) {
  if (n == 0) return SK_OK;
  std::vector<int> len(n);
  for (size_t k = 0, r = 0; k < (size_t)n; r += n_rows ? n_rows[k] : 1, ++k) {
    if (!rows[r]) return fail(ctx, SK_ERR_INVALID, "null sequence");
    len[k] = (int)std::strlen(rows[r]);
  }
  const bool no_lp = (flags & SK_FOLD_NO_LONELY_PAIRS) != 0;
  const size_t ns = sm ? (size_t)sm->n_samples : 0;
  const bool want_str = sm && sm->structs;
  sk::FoldLaunch L;
  std::vector<double> tab;
  L.no_gu = (flags & SK_FOLD_NO_GU) ? 1 : 0;
  L.no_closing_gu = (flags & SK_FOLD_NO_CLOSING_GU) ? 1 : 0;
  L.inside_only = sm ? 1 : 0;
  // the device memory one batch's tables may take (experiments build:
  // SK_FOLD_BUDGET gives it in bytes, so a test can split a small call)
  size_t free_b = 0, total_b = 0;
  SK_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
  double budget = std::min(16e9, 0.4 * (double)free_b);
  if (const char* e = SK_KNOB("SK_FOLD_BUDGET")) budget = std::atof(e);
  // experiments build: SK_FOLD_PATH = hbm | gtab keeps the launches off the LDS
  // ring / also leaves the hairpin and scale tables in HBM, so a test can run
  // those kernels on short items (read per call)
  if (const char* e = SK_KNOB("SK_FOLD_PATH")) {
    if (!std::strcmp(e, "hbm")) L.min_path = sk::kFoldPathHbm;
    else if (!std::strcmp(e, "gtab")) L.min_path = sk::kFoldPathGtab;
    else return fail(ctx, SK_ERR_INVALID, "SK_FOLD_PATH: hbm or gtab");
  }
  const bool stats = std::getenv("SK_HOST_STATS") != nullptr;
  hipStream_t S = ctx->stream;
  size_t out_host = 0;  // packed outputs of the batches before (host)
  size_t str_host = 0;  // sampled structures written so far (host)
  size_t row = 0;       // first row of item b0 in rows
  int n_batches = 0;
  for (int32_t b0 = 0; b0 < n; ++n_batches) {
    // (the sampled structures of the batch count too: n_samples chars per nucleotide)
    const int32_t b1 = sk::fold_batch_end(b0, n, budget, [&](int32_t k) {
      return (double)sk::FoldWork::doubles(K.tables, (size_t)len[k]) * 8.0 +
             K.more_bytes((double)len[k], n_rows ? (double)n_rows[k] : 1.0, no_lp) +
             (want_str ? (double)len[k] * (double)ns : 0.0);
    });
    std::vector<sk::FoldSeq> sq;
    std::vector<int8_t> codes;
    std::vector<uint8_t> lp;  // --noLonelyPairs tables
    size_t work = 0, outn = 0;
    int bmax = 0;
    for (int32_t k = b0; k < b1; ++k) {
      const size_t nn = (size_t)len[k];
      sk::FoldSeq f;
      f.seq_off = (int64_t)codes.size();
      f.work_off = (int64_t)work;
      f.out_off = (int64_t)outn;
      f.n = (int32_t)nn;
      f.n_rows = n_rows ? n_rows[k] : 1;
      codes.resize(codes.size() + (size_t)f.n_rows * nn);
      for (int32_t r = 0; r < f.n_rows; ++r, ++row) sk::fold_codes(rows[row], nn, codes.data() + f.seq_off + r * nn);
      if (no_lp) {
        f.lp_off = (int64_t)lp.size();
        lp.resize(lp.size() + nn * nn);
        K.lonely(codes.data() + f.seq_off, f.n_rows, (int)nn, L.no_gu != 0, lp.data() + f.lp_off);
      }
      work += sk::FoldWork::doubles(K.tables, nn);
      outn += nn > 1 ? nn * (nn - 1) / 2 : 0;
      bmax = std::max(bmax, (int)nn);
      sq.push_back(f);
    }
    const int nb = b1 - b0;
    sk::fold_tables(bmax, L, tab);  // sized by this batch's longest item
    if (K.more_tables) K.more_tables(L, tab);
    if (K.lds_bytes(L, bmax) > sk::kFoldLdsMax) return fail(ctx, SK_ERR_UNSUPPORTED, K.too_long);
    if (sm && sk::fold_sample_lds_bytes(L, bmax) > sk::kFoldLdsMax)
      return fail(ctx, SK_ERR_UNSUPPORTED, "fold: sequence too long for the sampling kernel's LDS");
    const size_t strn = want_str ? codes.size() * ns : 0;  // sampled structures, chars
    const size_t need = sq.size() * sizeof(sk::FoldSeq) + codes.size() + lp.size() + tab.size() * 8 +
                        (outn + nb) * 8 + strn + 10 * 256;
    int rc = ensure_work(ctx, need);
    if (rc) return rc;
    rc = ensure_scratch(ctx, std::max<size_t>(work * 8, 64));
    if (rc) return rc;
    Arena A{static_cast<char*>(ctx->work), 0, ctx->work_bytes};
    sk::FoldSeq* d_sq = A.take<sk::FoldSeq>(sq.size());
    int8_t* d_codes = A.take<int8_t>(std::max<size_t>(codes.size(), 1));
    double* d_tab = A.take<double>(tab.size());
    double* d_out = A.take<double>(std::max<size_t>(outn, 1));
    double* d_lz = A.take<double>(nb);
    uint8_t* d_lp = no_lp ? A.take<uint8_t>(std::max<size_t>(lp.size(), 1)) : nullptr;
    if (no_lp && !lp.empty())
      SK_HIP(ctx, hipMemcpyAsync(d_lp, lp.data(), lp.size(), hipMemcpyHostToDevice, S));
    SK_HIP(ctx, hipMemcpyAsync(d_sq, sq.data(), sq.size() * sizeof(sk::FoldSeq), hipMemcpyHostToDevice, S));
    if (!codes.empty())
      SK_HIP(ctx, hipMemcpyAsync(d_codes, codes.data(), codes.size(), hipMemcpyHostToDevice, S));
    SK_HIP(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, S));
    SK_HIP(ctx, hipMemsetAsync(ctx->scratch, 0, work * 8, S));
    SK_HIP(ctx, hipMemsetAsync(d_out, 0, std::max<size_t>(outn, 1) * 8, S));
    // sampling: d_out holds the uint32 pair counts (zeroed above)
    char* d_str = want_str ? A.take<char>(std::max<size_t>(strn, 1)) : nullptr;
    int32_t* d_status = sm ? A.take<int32_t>(1) : nullptr;
    if (want_str && strn) SK_HIP(ctx, hipMemsetAsync(d_str, '.', strn, S));
    if (sm) SK_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(int32_t), S));
    L.seqs = d_sq;
    L.codes = d_codes;
    L.tab = d_tab;
    L.lp = d_lp;
    L.work = ctx->scratch;
    L.out = d_out;
    L.log_z = d_lz;
    if (stats)
      std::fprintf(stderr, "[sk] fold batch: %d items, longest %d, path %s\n", nb, bmax,
                   sk::fold_path_name(K.path(L, bmax)));
    SK_HIP(ctx, K.launch(L, nb, bmax, S));
    std::vector<double> lz(nb);
    std::vector<uint32_t> cnt;
    int32_t status = 0;
    if (sm) {
      sk::FoldSampleLaunch SL;
      SL.F = L;
      SL.cnt = reinterpret_cast<uint32_t*>(d_out);
      SL.structs = d_str;
      SL.status = d_status;
      SL.n_samples = sm->n_samples;
      SL.seq_base = b0;
      SL.seed = sm->seed;
      SK_HIP(ctx, sk::launch_fold_sample(SL, nb, bmax, S));
      if (out && outn) {
        cnt.resize(outn);
        SK_HIP(ctx, hipMemcpyAsync(cnt.data(), d_out, outn * 4, hipMemcpyDeviceToHost, S));
      }
      if (strn) SK_HIP(ctx, hipMemcpyAsync(sm->structs + str_host, d_str, strn, hipMemcpyDeviceToHost, S));
      SK_HIP(ctx, hipMemcpyAsync(&status, d_status, sizeof(int32_t), hipMemcpyDeviceToHost, S));
    } else if (outn) {
      SK_HIP(ctx, hipMemcpyAsync(out + out_host, d_out, outn * 8, hipMemcpyDeviceToHost, S));
    }
    SK_HIP(ctx, hipMemcpyAsync(lz.data(), d_lz, nb * 8, hipMemcpyDeviceToHost, S));
    SK_HIP(ctx, hipStreamSynchronize(S));
    for (int k = 0; k < nb; ++k) {
      if (!std::isfinite(lz[k])) return fail(ctx, SK_ERR_UNSUPPORTED, K.out_of_range);
      if (log_z) log_z[b0 + k] = lz[k];
    }
    if (status == sk::kFoldSampleRunaway)
      return fail(ctx, SK_ERR_HIP, "fold sampling: a walk made more than 2 n + 2 decisions");
    if (status == sk::kFoldSampleNoWeight)
      return fail(ctx, SK_ERR_HIP, "fold sampling: a decision's candidates sum to 0 or a non-finite value");
    if (status != 0) return fail(ctx, SK_ERR_HIP, "fold sampling: more open segments than the stack holds");
    // bpp = count / n_samples (common/bpmatrix.cpp:220-226)
    for (size_t a = 0; a < cnt.size(); ++a) out[out_host + a] = (double)cnt[a] / (double)ns;
    out_host += outn;
    str_host += strn;
    b0 = b1;
  }
  if (stats) std::fprintf(stderr, "[sk] fold: %d items in %d batches\n", (int)n, n_batches);
  return SK_OK;
}

// sk_dataset_add_folded (n_samples = 0) and sk_dataset_add_sampled
int add_folded(sk_context* ctx, sk_dataset* ds, int32_t n, int32_t n_rows, const char* const* rows,
               const char* const* labels, float th, int32_t fold_flags, int32_t n_samples, uint64_t seed,
               int32_t n_threads) {
  if (!ctx || !ds || n < 0 || n_rows < 1 || (n > 0 && !rows)) return fail(ctx, SK_ERR_INVALID, "null argument");
  if (ds->uploaded) return fail(ctx, SK_ERR_INVALID, "dataset already uploaded");
  if (ds_mixes(ds, kSortRna)) return fail(ctx, SK_ERR_INVALID, ds->err);
  const size_t nr = (size_t)n * n_rows;
  // fold the gap-erased, lower-cased rows (common/bpmatrix.cpp:404-414)
  std::vector<std::string> erased(nr);
  std::vector<const char*> eptr(nr);
  std::vector<size_t> off(nr + 1, 0);
  for (size_t r = 0; r < nr; ++r) {
    if (!rows[r]) return fail(ctx, SK_ERR_INVALID, "null row");
    for (const char* p = rows[r]; *p; ++p)
      if (*p != '-') erased[r].push_back((char)std::tolower((unsigned char)*p));
    eptr[r] = erased[r].c_str();
    const size_t m = erased[r].size();
    off[r + 1] = off[r] + (m > 1 ? m * (m - 1) / 2 : 0);
  }
  std::vector<double> bpp(std::max<size_t>(off[nr], 1));
  int rc = n_samples > 0 ? sk_fold_sample(ctx, (int32_t)nr, eptr.data(), fold_flags, n_samples, seed, bpp.data(),
                                          nullptr, nullptr)
                         : sk_fold_mccaskill(ctx, (int32_t)nr, eptr.data(), fold_flags, bpp.data(), nullptr);
  if (rc) return rc;
  std::vector<const double*> bptr(nr);
  for (size_t r = 0; r < nr; ++r) bptr[r] = bpp.data() + off[r];
  rc = add_examples_threaded(ds, n, n_rows, rows, bptr.data(), labels, th, 1, n_threads);
  return rc ? fail(ctx, rc, "example build failed") : SK_OK;
}
}  // namespace

}  // namespace sk

extern "C" {

int sk_fold_mccaskill(sk_context* ctx, int32_t n, const char* const* seqs, int32_t flags,
                      double* out, double* log_z) {
  if (!ctx || n < 0 || (n > 0 && (!seqs || !out))) return sk::fail(ctx, SK_ERR_INVALID, "null argument");
  if (flags & ~(SK_FOLD_NO_GU | SK_FOLD_NO_CLOSING_GU | SK_FOLD_NO_LONELY_PAIRS))
    return sk::fail(ctx, SK_ERR_UNSUPPORTED, "fold: unknown flag");
  return sk::fold_batches(ctx, sk::kFoldPlain, n, nullptr, seqs, flags, out, log_z, nullptr);
}

int sk_fold_sample(sk_context* ctx, int32_t n, const char* const* seqs, int32_t flags,
                   int32_t n_samples, uint64_t seed, double* out_bpp, char* out_structs, double* log_z) {
  if (!ctx || n < 0 || (n > 0 && !seqs)) return sk::fail(ctx, SK_ERR_INVALID, "null argument");
  if (n_samples < 1) return sk::fail(ctx, SK_ERR_INVALID, "fold sampling: n_samples must be at least 1");
  if (!out_bpp && !out_structs) return sk::fail(ctx, SK_ERR_INVALID, "fold sampling: no output asked for");
  if (flags & ~(SK_FOLD_NO_GU | SK_FOLD_NO_CLOSING_GU | SK_FOLD_NO_LONELY_PAIRS))
    return sk::fail(ctx, SK_ERR_UNSUPPORTED, "fold: unknown flag");
  sk::FoldSampling sm;
  sm.n_samples = n_samples;
  sm.seed = seed;
  sm.structs = out_structs;
  return sk::fold_batches(ctx, sk::kFoldPlain, n, nullptr, seqs, flags, out_bpp, log_z, &sm);
}

double sk_fold_sample_uniform(uint64_t seed, int32_t seq, int32_t sample, int32_t draw) {
  return sk::rng_uniform(sk::rng_stream(seed, seq, sample), draw);
}

int sk_fold_alignment(sk_context* ctx, int32_t n_aln, const int32_t* n_rows, const char* const* rows,
                      int32_t flags, double* out, double* log_z) {
  if (!ctx || n_aln < 0 || (n_aln > 0 && (!n_rows || !rows || !out))) return sk::fail(ctx, SK_ERR_INVALID, "null argument");
  if (flags & ~(SK_FOLD_NO_GU | SK_FOLD_NO_CLOSING_GU | SK_FOLD_NO_LONELY_PAIRS))
    return sk::fail(ctx, SK_ERR_UNSUPPORTED, "fold: unknown flag");
  if (flags & SK_FOLD_NO_CLOSING_GU)
    return sk::fail(ctx, SK_ERR_UNSUPPORTED,
                "consensus fold: --noClosingGU has no per-column meaning when the rows differ");
  size_t r = 0;  // row in rows
  for (int32_t k = 0, len = 0; k < n_aln; ++k) {
    if (n_rows[k] < 1) return sk::fail(ctx, SK_ERR_INVALID, "consensus fold: an alignment needs at least one row");
    if (n_rows[k] > sk::kAliMaxRows) return sk::fail(ctx, SK_ERR_UNSUPPORTED, "consensus fold: too many rows");
    for (int32_t a = 0; a < n_rows[k]; ++a, ++r) {
      if (!rows[r]) return sk::fail(ctx, SK_ERR_INVALID, "null row");
      const int m = (int)std::strlen(rows[r]);
      if (a == 0) len = m;
      else if (m != len) return sk::fail(ctx, SK_ERR_INVALID, "consensus fold: rows of unequal length");
    }
  }
  return sk::fold_batches(ctx, sk::kFoldAli, n_aln, n_rows, rows, flags, out, log_z, nullptr);
}

int sk_dataset_add_folded(sk_context* ctx, sk_dataset* ds, int32_t n, int32_t n_rows,
                          const char* const* rows, const char* const* labels, float th,
                          int32_t fold_flags, int32_t n_threads) {
  return sk::add_folded(ctx, ds, n, n_rows, rows, labels, th, fold_flags, 0, 0, n_threads);
}

int sk_dataset_add_sampled(sk_context* ctx, sk_dataset* ds, int32_t n, int32_t n_rows,
                           const char* const* rows, const char* const* labels, float th,
                           int32_t fold_flags, int32_t n_samples, uint64_t seed, int32_t n_threads) {
  if (n_samples < 1) return sk::fail(ctx, SK_ERR_INVALID, "fold sampling: n_samples must be at least 1");
  return sk::add_folded(ctx, ds, n, n_rows, rows, labels, th, fold_flags, n_samples, seed, n_threads);
}

int sk_dataset_add_alifolded(sk_context* ctx, sk_dataset* ds, int32_t n, int32_t n_rows,
                             const char* const* rows, const char* const* labels, float th,
                             int32_t fold_flags, int32_t n_threads) {
  if (!ctx || !ds || n < 0 || n_rows < 1 || (n > 0 && !rows)) return sk::fail(ctx, SK_ERR_INVALID, "null argument");
  if (ds->uploaded) return sk::fail(ctx, SK_ERR_INVALID, "dataset already uploaded");
  if (sk::ds_mixes(ds, sk::kSortRna)) return sk::fail(ctx, SK_ERR_INVALID, ds->err);
  // one consensus matrix per example, in alignment coordinates
  std::vector<size_t> off((size_t)n + 1, 0);
  for (int32_t i = 0; i < n; ++i) {
    if (!rows[(size_t)i * n_rows]) return sk::fail(ctx, SK_ERR_INVALID, "null row");
    const size_t m = std::strlen(rows[(size_t)i * n_rows]);
    off[i + 1] = off[i] + (m > 1 ? m * (m - 1) / 2 : 0);
  }
  std::vector<double> bpp(std::max<size_t>(off[n], 1));
  const std::vector<int32_t> nr((size_t)n, n_rows);
  int rc = sk_fold_alignment(ctx, n, nr.data(), rows, fold_flags, bpp.data(), nullptr);
  if (rc) return rc;
  std::vector<const double*> bptr((size_t)n);
  for (int32_t i = 0; i < n; ++i) bptr[i] = bpp.data() + off[i];
  rc = sk::add_examples_threaded(ds, n, n_rows, rows, bptr.data(), labels, th, 1, n_threads, true);
  return rc ? sk::fail(ctx, rc, "example build failed") : SK_OK;
}

int sk_dataset_add_palindromes_folded(sk_context* ctx, sk_dataset* ds, int32_t n, const char* const* seqs,
                                      const char* const* labels, int32_t fold_flags, int32_t seed_length,
                                      int32_t min_loop, int32_t max_dist, int32_t n_threads) {
  if (!ctx || !ds || n < 0 || (n > 0 && !seqs)) return sk::fail(ctx, SK_ERR_INVALID, "null argument");
  if (ds->uploaded) return sk::fail(ctx, SK_ERR_INVALID, "dataset already uploaded");
  if (sk::ds_mixes(ds, sk::kSortPal)) return sk::fail(ctx, SK_ERR_INVALID, ds->err);
  // the lowercased sequences (load_examples, simpal/simpal.cpp:298), folded as they are
  std::vector<std::string> low((size_t)n);
  std::vector<const char*> lptr((size_t)n);
  std::vector<size_t> off((size_t)n + 1, 0);
  for (int32_t i = 0; i < n; ++i) {
    if (!seqs[i]) return sk::fail(ctx, SK_ERR_INVALID, "null sequence");
    low[(size_t)i] = sk::lower(seqs[i]);
    lptr[(size_t)i] = low[(size_t)i].c_str();
    const size_t m = low[(size_t)i].size();
    const int rc = sk::pal_args(m, seed_length, min_loop, max_dist, &ds->err);
    if (rc) return sk::fail(ctx, rc, ds->err);
    off[(size_t)i + 1] = off[(size_t)i] + (m > 1 ? m * (m - 1) / 2 : 0);
  }
  if (sk::pal_seed_differs(ds, seed_length)) return sk::fail(ctx, SK_ERR_INVALID, ds->err);
  std::vector<double> bpp(std::max<size_t>(off[(size_t)n], 1));
  int rc = sk_fold_mccaskill(ctx, n, lptr.data(), fold_flags, bpp.data(), nullptr);
  if (rc) return rc;
  const size_t base = ds->ex.size();
  try {
    ds->ex.resize(base + (size_t)n);
    for (int32_t i = 0; i < n; ++i) ds->labels.emplace_back(labels && labels[i] ? labels[i] : "+1");
  } catch (const std::bad_alloc&) {
    return sk::fail(ctx, SK_ERR_ALLOC, "palindrome examples");
  }
  int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
  nt = std::max(1, std::min(nt, std::max<int32_t>(n, 1)));
  std::atomic<int32_t> next(0), status(SK_OK);
  auto work = [&]() {
    for (;;) {
      const int32_t i = next.fetch_add(1);
      if (i >= n || status.load() != SK_OK) return;
      try {
        sk::build_palindromes(ds->ex[base + (size_t)i], low[(size_t)i], bpp.data() + off[(size_t)i], seed_length,
                          min_loop, max_dist);
      } catch (...) {
        status.store(SK_ERR_ALLOC);
      }
    }
  };
  sk::run_pool(nt, work);
  if (status.load() != SK_OK) {
    ds->ex.resize(base);
    ds->labels.resize(base);
    return sk::fail(ctx, status.load(), "palindrome example build failed");
  }
  return SK_OK;
}

}  // extern "C"
