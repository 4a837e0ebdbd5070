// Datasets on the host: creating one, adding RNA, protein and palindrome
// examples (one by one, in threaded batches, synthetic ones) and reading an
// example's shape, DAG, profile and palindromes back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "host/runtime_types.h"
#include "blosum62.inc"

namespace sk {
namespace {
// a c g u -> 0 1 2 3 (the strings' order), anything else -1
int pal_code(char c) {
  switch (c) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 'u': return 3;
    default: return -1;
  }
}
}  // namespace

// char2aa (common/aaprofile.cpp:13-23)
int char2aa(int c) {
  if (c < 0 || c > 255) return 23;
  const int u = std::toupper(c);
  for (int k = 0; k < 23; ++k)
    if (SK_AA_LETTERS[k] == u) return k;
  return 23;
}

// arguments the builders refuse; the message in *err
int pal_args(size_t n, int32_t seed_length, int32_t min_loop, int32_t max_dist, std::string* err) {
  if (seed_length < 1 || seed_length > 32) {
    *err = "palindrome seed_length outside 1..32";
    return SK_ERR_UNSUPPORTED;
  }
  if (min_loop < 0 || max_dist < 0) {
    *err = "negative min_loop or max_dist";
    return SK_ERR_INVALID;
  }
  if (n < (size_t)seed_length) {  // the reference's loop bound wraps (simpal.cpp:116)
    *err = "sequence shorter than seed_length";
    return SK_ERR_INVALID;
  }
  return SK_OK;
}
// Pals::make_pal_map (simpal/simpal.cpp:101-218) over the lowercased
// sequence seq and its bpp (packed strict upper, double).  Same (key, d)
// weights are added in float in the order increasing i, then increasing r.
void build_palindromes(Example& ex, const std::string& seq, const double* bpp, int32_t s, int32_t min_loop,
                       int32_t max_dist) {
  const int n = (int)seq.size();
  ex = Example();
  ex.pal = true;
  ex.pal_seed = s;
  ex.len = n;
  ex.n_rows = 1;
  ex.n_seqs = 1.0f;
  ex.rows.assign(1, seq);
  // k-mers i in [0, n - s) (the last one is skipped, :116) as 2-bit words,
  // forward and of the reversed complement (RevComp, :73-95: t pairs as u,
  // anything else maps to NUL and never matches)
  const int nk = n - s;
  const size_t nks = (size_t)std::max(nk, 0);
  std::vector<uint64_t> fk(nks), rk(nks);
  std::vector<uint8_t> fok(nks), rok(nks);
  auto comp = [](char c) {
    switch (c) {
      case 'a': return 3;
      case 'c': return 2;
      case 'g': return 1;
      case 'u':
      case 't': return 0;
      default: return -1;
    }
  };
  for (int i = 0; i < nk; ++i) {
    uint64_t kf = 0, kr = 0;
    bool okf = true, okr = true;
    for (int t = 0; t < s; ++t) {
      const int a = pal_code(seq[(size_t)(i + t)]), b = comp(seq[(size_t)(n - 1 - i - t)]);
      okf = okf && a >= 0;
      okr = okr && b >= 0;
      kf = (kf << 2) | (uint64_t)(a & 3);
      kr = (kr << 2) | (uint64_t)(b & 3);
    }
    fk[(size_t)i] = kf;
    rk[(size_t)i] = kr;
    fok[(size_t)i] = okf;
    rok[(size_t)i] = okr;
  }
  std::map<std::pair<uint64_t, int32_t>, float> pals;
  for (int i = 0; i < nk; ++i) {
    if (!fok[(size_t)i]) continue;
    for (int r = 0; r < nk; ++r) {
      if (!rok[(size_t)r] || rk[(size_t)r] != fk[(size_t)i]) continue;
      const int d = n - i - r - 2 * s;  // unsigned in the reference (:152): negative fails
      if (d < min_loop || d > max_dist) continue;
      float weight = 1.0f;
      for (int t = 0; t < s; ++t) {
        // pf(m, n) with m = i + 1 + t < n = len - r - t, 1-based (:170-171),
        // the double rounded to float (PFWrapper::operator(), pf_wrapper.h:41-44)
        const float p = (float)bpp[sk::tri_index(n, i + t, n - r - t - 1)];
        weight = p * weight;
      }
      auto it = pals.find(std::make_pair(fk[(size_t)i], (int32_t)d));
      if (it == pals.end())
        pals.emplace(std::make_pair(fk[(size_t)i], (int32_t)d), weight);
      else
        it->second += weight;
    }
  }
  for (const auto& e : pals) {
    ex.pal_key.push_back(e.first.first);
    ex.pal_dist.push_back(e.first.second);
    ex.pal_w.push_back(e.second);
  }
}
std::string lower(const char* s) {
  std::string o(s);
  for (char& c : o) c = (char)std::tolower((unsigned char)c);
  return o;
}

// Threaded DAG builds of n examples of n_rows rows from per-row bpp (caller's
// or folded), appended to ds; the parallel form of the reference's load loop
// (common/framework.h:308-353 + DataLoader<MData>::get, data.cpp:548-586).
// (consensus: bpp_rows[i] is example i's one matrix in alignment coordinates)
int add_examples_threaded(sk_dataset* ds, int32_t n, int32_t n_rows, const char* const* rows,
                          const double* const* bpp_rows, const char* const* labels, float th,
                          int use_bp, int32_t n_threads, bool consensus) {
  if (ds_mixes(ds, kSortRna)) return SK_ERR_INVALID;
  const size_t base = ds->ex.size();
  try {
    ds->ex.resize(base + n);
    for (int32_t i = 0; i < n; ++i) ds->labels.emplace_back(labels && labels[i] ? labels[i] : "+1");
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
  int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
  nt = std::max(1, std::min(nt, std::max<int32_t>(n, 1)));
  std::atomic<int32_t> next(0), status(SK_OK);
  auto work = [&]() {
    for (;;) {
      const int32_t i = next.fetch_add(1);
      if (i >= n || status.load() != SK_OK) return;
      try {
        sk::build_example(ds->ex[base + i], n_rows, rows + (size_t)i * n_rows,
                          use_bp ? bpp_rows + (size_t)i * (consensus ? 1 : n_rows) : nullptr, th, use_bp != 0,
                          consensus);
      } catch (...) {
        status.store(SK_ERR_INVALID);
      }
    }
  };
  run_pool(nt, work);
  if (status.load() != SK_OK) {
    ds->ex.resize(base);
    ds->labels.resize(base);
  }
  return status.load();
}

}  // namespace sk

extern "C" {

int sk_dataset_create(sk_dataset** ds) {
  if (!ds) return SK_ERR_INVALID;
  *ds = new (std::nothrow) sk_dataset();
  return *ds ? SK_OK : SK_ERR_ALLOC;
}

int sk_dataset_free(sk_dataset* ds) {
  delete ds;
  return SK_OK;
}

int sk_dataset_add(sk_dataset* ds, const char* label, int n_rows, const char* const* rows,
                   const double* const* bpp_rows, float th, int use_bp) {
  if (!ds || n_rows <= 0 || !rows) return SK_ERR_INVALID;
  if (use_bp && !bpp_rows) return SK_ERR_INVALID;
  if (ds->uploaded || sk::ds_mixes(ds, sk::kSortRna)) return SK_ERR_INVALID;
  try {
    sk::Example ex;
    sk::build_example(ex, n_rows, rows, bpp_rows, th, use_bp != 0);
    ds->ex.push_back(std::move(ex));
    ds->labels.emplace_back(label ? label : "");
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  } catch (const std::exception& e) {
    ds->err = e.what();
    return SK_ERR_INVALID;
  }
  return SK_OK;
}

int sk_dataset_add_consensus(sk_dataset* ds, const char* label, int n_rows, const char* const* rows,
                             const double* bpp, float th) {
  if (!ds || n_rows <= 0 || !rows || !bpp) return SK_ERR_INVALID;
  if (ds->uploaded || sk::ds_mixes(ds, sk::kSortRna)) return SK_ERR_INVALID;
  try {
    sk::Example ex;
    sk::build_example(ex, n_rows, rows, &bpp, th, true, true);
    ds->ex.push_back(std::move(ex));
    ds->labels.emplace_back(label ? label : "");
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  } catch (const std::exception& e) {
    ds->err = e.what();
    return SK_ERR_INVALID;
  }
  return SK_OK;
}

int sk_dataset_add_protein(sk_dataset* ds, const char* label, int n_rows, const char* const* rows) {
  if (!ds || n_rows <= 0 || !rows) return SK_ERR_INVALID;
  if (ds->uploaded || sk::ds_mixes(ds, sk::kSortProtein)) return SK_ERR_INVALID;
  if (n_rows >= sk::kAaMaxRows) {
    ds->err = "protein alignments of 4,096 rows or more are not supported";
    return SK_ERR_UNSUPPORTED;
  }
  for (int r = 0; r < n_rows; ++r)
    if (!rows[r]) return SK_ERR_INVALID;
  try {
    sk::Example ex;
    const size_t L = std::strlen(rows[0]);
    for (int r = 1; r < n_rows; ++r)
      if (std::strlen(rows[r]) != L) {
        ds->err = "wrong alignment";  // bpla_kernel/data.cpp:284-288
        return SK_ERR_INVALID;
      }
    ex.protein = true;
    ex.len = (int)L;
    ex.n_rows = n_rows;
    ex.n_seqs = (float)n_rows;
    ex.aa_prof.assign(L * sk::kAaSlots, 0.0f);
    for (int r = 0; r < n_rows; ++r) {
      ex.rows.emplace_back(rows[r]);
      // AAProfileSequence::add_sequence, weight 1 (common/aaprofile.cpp:49-60)
      for (size_t i = 0; i < L; ++i) ex.aa_prof[i * sk::kAaSlots + sk::char2aa((unsigned char)rows[r][i])] += 1.0f;
    }
    ds->ex.push_back(std::move(ex));
    ds->labels.emplace_back(label ? label : "");
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
  return SK_OK;
}

int sk_dataset_aa_profile(const sk_dataset* ds, int i, float* prof24, float* n_seqs) {
  if (!ds) return SK_ERR_INVALID;
  if (i < 0 || i >= (int)ds->ex.size()) return SK_ERR_RANGE;
  const sk::Example& X = ds->ex[i];
  if (!X.protein) return SK_ERR_INVALID;
  if (prof24) std::copy(X.aa_prof.begin(), X.aa_prof.end(), prof24);
  if (n_seqs) *n_seqs = X.n_seqs;
  return SK_OK;
}

int sk_dataset_add_palindromes(sk_dataset* ds, const char* label, const char* seq, const double* bpp,
                               int32_t seed_length, int32_t min_loop, int32_t max_dist) {
  if (!ds || !seq) return SK_ERR_INVALID;
  if (ds->uploaded || sk::ds_mixes(ds, sk::kSortPal)) return SK_ERR_INVALID;
  try {
    const std::string sq = sk::lower(seq);
    const int rc = sk::pal_args(sq.size(), seed_length, min_loop, max_dist, &ds->err);
    if (rc) return rc;
    if (sk::pal_seed_differs(ds, seed_length)) return SK_ERR_INVALID;
    if (!bpp && sq.size() > 1) return SK_ERR_INVALID;
    sk::Example ex;
    sk::build_palindromes(ex, sq, bpp, seed_length, min_loop, max_dist);
    ds->ex.push_back(std::move(ex));
    ds->labels.emplace_back(label ? label : "");
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
  return SK_OK;
}

int sk_dataset_add_palindrome_entries(sk_dataset* ds, const char* label, int32_t seed_length, int32_t n,
                                      const char* keys, const int32_t* dist, const float* weight) {
  if (!ds || n < 0 || (n > 0 && (!keys || !dist || !weight))) return SK_ERR_INVALID;
  if (ds->uploaded || sk::ds_mixes(ds, sk::kSortPal)) return SK_ERR_INVALID;
  if (seed_length < 1 || seed_length > 32) {
    ds->err = "palindrome seed_length outside 1..32";
    return SK_ERR_UNSUPPORTED;
  }
  if (sk::pal_seed_differs(ds, seed_length)) return SK_ERR_INVALID;
  try {
    struct Ent {
      uint64_t key;
      int32_t dist;
      float w;
    };
    std::vector<Ent> v((size_t)n);
    for (int32_t k = 0; k < n; ++k) {
      uint64_t key = 0;
      for (int t = 0; t < seed_length; ++t) {
        const int c = sk::pal_code(keys[(size_t)k * seed_length + t]);
        if (c < 0) {
          ds->err = "palindrome key letter outside acgu";
          return SK_ERR_INVALID;
        }
        key = (key << 2) | (uint64_t)c;
      }
      if (dist[k] < 0 || !(weight[k] >= 0.0f) || !std::isfinite(weight[k])) {
        ds->err = "palindrome entry with a negative dist or a weight that is not finite and non-negative";
        return SK_ERR_INVALID;
      }
      v[(size_t)k] = Ent{key, dist[k], weight[k]};
    }
    std::sort(v.begin(), v.end(),
              [](const Ent& a, const Ent& b) { return a.key != b.key ? a.key < b.key : a.dist < b.dist; });
    for (size_t k = 1; k < v.size(); ++k)
      if (v[k].key == v[k - 1].key && v[k].dist == v[k - 1].dist) {
        ds->err = "duplicate palindrome entry (key, dist)";
        return SK_ERR_INVALID;
      }
    sk::Example ex;
    ex.pal = true;
    ex.pal_seed = seed_length;
    ex.n_rows = 1;
    ex.n_seqs = 1.0f;
    ex.rows.assign(1, std::string());
    for (const Ent& e : v) {
      ex.pal_key.push_back(e.key);
      ex.pal_dist.push_back(e.dist);
      ex.pal_w.push_back(e.w);
    }
    ds->ex.push_back(std::move(ex));
    ds->labels.emplace_back(label ? label : "");
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
  return SK_OK;
}

int sk_dataset_palindromes(const sk_dataset* ds, int i, int32_t* n, char* keys, int32_t* dist, float* weight) {
  if (!ds) return SK_ERR_INVALID;
  if (i < 0 || i >= (int)ds->ex.size()) return SK_ERR_RANGE;
  const sk::Example& X = ds->ex[i];
  if (!X.pal) return SK_ERR_INVALID;
  const size_t m = X.pal_key.size();
  if (n) *n = (int32_t)m;
  if (keys)
    for (size_t k = 0; k < m; ++k)
      for (int t = 0; t < X.pal_seed; ++t)
        keys[k * X.pal_seed + t] = "acgu"[(X.pal_key[k] >> (2 * (X.pal_seed - 1 - t))) & 3];
  if (dist) std::copy(X.pal_dist.begin(), X.pal_dist.end(), dist);
  if (weight) std::copy(X.pal_w.begin(), X.pal_w.end(), weight);
  return SK_OK;
}

int sk_dataset_add_synthetic_rows(sk_dataset* ds, int32_t n, int32_t n_rows,
                                  const char* const* rows, const char* const* labels, float th,
                                  int32_t n_threads) {
  if (!ds || n < 0 || n_rows < 1 || (n > 0 && !rows)) return SK_ERR_INVALID;
  if (ds->uploaded || sk::ds_mixes(ds, sk::kSortRna)) return SK_ERR_INVALID;
  const size_t base = ds->ex.size();
  try {
    ds->ex.resize(base + n);
    for (int32_t i = 0; i < n; ++i) ds->labels.emplace_back(labels && labels[i] ? labels[i] : "+1");
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
  int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
  nt = std::max(1, std::min(nt, std::max<int32_t>(n, 1)));
  std::atomic<int32_t> next(0), status(SK_OK);
  static const bool stats = std::getenv("SK_HOST_STATS") != nullptr;
  std::atomic<int64_t> ns_fold(0), ns_build(0);
  auto work = [&]() {
    std::vector<std::vector<double>> bpp(n_rows);
    std::vector<const double*> bptr(n_rows);
    for (;;) {
      const int32_t i = next.fetch_add(1);
      if (i >= n || status.load() != SK_OK) return;
      try {
        const auto t0 = std::chrono::steady_clock::now();
        const char* const* ex_rows = rows + (size_t)i * n_rows;
        for (int32_t r = 0; r < n_rows; ++r) {
          const char* s = ex_rows[r];
          const int L = (int)std::strlen(s);
          // fold the gap-erased, lower-cased row (common/bpmatrix.cpp:404-414)
          std::string row;
          for (int k = 0; k < L; ++k)
            if (s[k] != '-') row.push_back((char)std::tolower((unsigned char)s[k]));
          bpp[r].assign(row.size() > 1 ? row.size() * (row.size() - 1) / 2 : 1, 0.0);
          sk::fold_nussinov(row.c_str(), (int)row.size(), false, bpp[r].data());
          bptr[r] = bpp[r].data();
        }
        const auto t1 = std::chrono::steady_clock::now();
        sk::build_example(ds->ex[base + i], n_rows, ex_rows, bptr.data(), th, true);
        if (stats) {
          const auto t2 = std::chrono::steady_clock::now();
          ns_fold += std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
          ns_build += std::chrono::duration_cast<std::chrono::nanoseconds>(t2 - t1).count();
        }
      } catch (...) {
        status.store(SK_ERR_INVALID);
      }
    }
  };
  sk::run_pool(nt, work);
  if (stats)
    std::fprintf(stderr, "[sk] synthetic examples: %d on %d threads, fold %.3f s, build %.3f s (thread-seconds)\n", n,
                 nt, ns_fold.load() * 1e-9, ns_build.load() * 1e-9);
  if (status.load() != SK_OK) {
    ds->ex.resize(base);
    ds->labels.resize(base);
  }
  return status.load();
}

int sk_dataset_add_synthetic(sk_dataset* ds, int32_t n, const char* const* seqs,
                             const char* const* labels, float th, int32_t n_threads) {
  return sk_dataset_add_synthetic_rows(ds, n, 1, seqs, labels, th, n_threads);
}

int sk_dataset_size(const sk_dataset* ds) { return ds ? (int)ds->ex.size() : 0; }

const char* sk_dataset_label(const sk_dataset* ds, int i) {
  if (!ds || i < 0 || i >= (int)ds->labels.size()) return nullptr;
  return ds->labels[i].c_str();
}

int sk_dataset_shape(const sk_dataset* ds, int i, int32_t* n_nodes, int32_t* n_edges,
                     int32_t* n_bpfreq, int32_t* n_roots, int32_t* seq_len) {
  if (!ds) return SK_ERR_INVALID;
  if (i < 0 || i >= (int)ds->ex.size()) return SK_ERR_RANGE;
  const sk::Example& X = ds->ex[i];
  if (n_nodes) *n_nodes = X.n_nodes();
  if (n_edges) *n_edges = X.n_edges();
  if (n_bpfreq) *n_bpfreq = (int32_t)X.bpf_code.size();
  if (n_roots) *n_roots = (int32_t)X.roots.size();
  if (seq_len) *seq_len = X.len;
  return SK_OK;
}

int sk_dataset_row_traffic(const sk_dataset* ds, int i, int32_t* rows, int32_t* stored,
                           int32_t* slab_reads, int32_t* gamma_reads, int32_t* phi_reads,
                           int32_t* reg_reads, int32_t* y_slots) {
  if (!ds) return SK_ERR_INVALID;
  if (i < 0 || i >= (int)ds->ex.size()) return SK_ERR_RANGE;
  const sk::HostPack& P = ds->pack;
  if ((int)P.ex_nlxg.size() != (int)ds->ex.size()) return SK_ERR_INVALID;  // not packed yet
  // the kernel's row reads: slab / Gamma / Phi child records, minus the
  // previous row's (taken from registers); stored rows (slot < 0x4000)
  int32_t st = 0, sl = 0, ga = 0, ph = 0, rg = 0;
  uint32_t prev = 0xffffu;
  // (of the schedule the kernel runs: the factored one where it was built)
  const auto& rows_ = P.run_rows();
  const auto& ch_ = P.run_ch();
  const int32_t nlr = P.run_nl()[i];
  size_t k = (size_t)P.run_ch_base()[i];
  for (size_t r = (size_t)P.run_base()[i]; r < (size_t)P.run_base()[i] + nlr; ++r) {
    const int ne = rows_[r].a & 0xff;
    for (int t = 0; t < ne; ++t, ++k) {
      const uint32_t c = ch_[k] & 0xffffu;
      if (c == prev) ++rg;
      else if (c & 0x8000u) ++ga;
      else if (c & 0x4000u) ++ph;
      else ++sl;
    }
    prev = rows_[r].b >> 16;
    st += prev < 0x4000u;
  }
  if (rows) *rows = nlr;
  if (stored) *stored = st;
  if (slab_reads) *slab_reads = sl;
  if (gamma_reads) *gamma_reads = ga;
  if (phi_reads) *phi_reads = ph;
  if (reg_reads) *reg_reads = rg;
  if (y_slots) *y_slots = P.ex_nl[i];
  return SK_OK;
}

int sk_dataset_shared_sums(const sk_dataset* ds, int i, int32_t* shared_rows, int32_t* member_records) {
  if (!ds) return SK_ERR_INVALID;
  if (i < 0 || i >= (int)ds->ex.size()) return SK_ERR_RANGE;
  const sk::HostPack& P = ds->pack;
  if ((int)P.ex_nlxg.size() != (int)ds->ex.size()) return SK_ERR_INVALID;  // not packed yet
  if (shared_rows) *shared_rows = P.shared_sums ? P.ex_ss_rows[i] : 0;
  if (member_records) *member_records = P.shared_sums ? P.ex_ss_repl[i] : 0;
  return SK_OK;
}

int sk_dataset_dag(const sk_dataset* ds, int i, uint32_t* first, uint32_t* last,
                   uint32_t* n_edges, uint32_t* n_bpfreq, float* weight, uint32_t* max_pa,
                   uint32_t* edge_to, uint32_t* edge_gaps, uint32_t* bp_code, float* bp_p,
                   uint32_t* roots, float* pos_weight) {
  if (!ds) return SK_ERR_INVALID;
  if (i < 0 || i >= (int)ds->ex.size()) return SK_ERR_RANGE;
  const sk::Example& X = ds->ex[i];
  const int n = X.n_nodes();
  for (int v = 0; v < n; ++v) {
    if (first) first[v] = X.first[v];
    if (last) last[v] = X.last[v];
    if (n_edges) n_edges[v] = X.edge_off[v + 1] - X.edge_off[v];
    if (n_bpfreq) n_bpfreq[v] = X.bpf_off[v + 1] - X.bpf_off[v];
    if (weight) weight[v] = X.weight[v];
    if (max_pa) max_pa[v] = X.max_pa[v];
  }
  if (edge_to) std::copy(X.edge_to.begin(), X.edge_to.end(), edge_to);
  if (edge_gaps) std::copy(X.edge_gaps.begin(), X.edge_gaps.end(), edge_gaps);
  if (bp_code) std::copy(X.bpf_code.begin(), X.bpf_code.end(), bp_code);
  if (bp_p) std::copy(X.bpf_p.begin(), X.bpf_p.end(), bp_p);
  if (roots) std::copy(X.roots.begin(), X.roots.end(), roots);
  if (pos_weight && X.has_bp) std::copy(X.pos_weight.begin(), X.pos_weight.end(), pos_weight);
  return SK_OK;
}

int sk_dataset_profile(const sk_dataset* ds, int i, float* prof5, float* n_seqs) {
  if (!ds) return SK_ERR_INVALID;
  if (i < 0 || i >= (int)ds->ex.size()) return SK_ERR_RANGE;
  const sk::Example& X = ds->ex[i];
  if (prof5) std::copy(X.prof5.begin(), X.prof5.end(), prof5);
  if (n_seqs) *n_seqs = X.n_seqs;
  return SK_OK;
}

int sk_dataset_bpla_weights(const sk_dataset* ds, int i, float* p_left, float* p_right,
                            float* p_unpair) {
  if (!ds) return SK_ERR_INVALID;
  if (i < 0 || i >= (int)ds->ex.size()) return SK_ERR_RANGE;
  const sk::Example& X = ds->ex[i];
  for (int k = 0; k < X.len; ++k) {
    const float4 w = sk::bpla_weight(X, k);
    if (p_left) p_left[k] = w.x;
    if (p_right) p_right[k] = w.y;
    if (p_unpair) p_unpair[k] = w.z;
  }
  return SK_OK;
}

int sk_dataset_add_batch(sk_dataset* ds, int32_t n, int32_t n_rows, const char* const* rows,
                         const double* const* bpp_rows, const char* const* labels, float th,
                         int32_t use_bp, int32_t n_threads) {
  if (!ds || n < 0 || n_rows < 1 || (n > 0 && (!rows || (use_bp && !bpp_rows)))) return SK_ERR_INVALID;
  if (ds->uploaded) return SK_ERR_INVALID;
  return sk::add_examples_threaded(ds, n, n_rows, rows, bpp_rows, labels, th, use_bp, n_threads);
}

}  // extern "C"
