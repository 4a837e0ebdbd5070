// Internals of the host runtime (not part of the ABI): the dataset and
// context structs behind the C handles, the packed host image, the helpers
// sk_api.cpp and the subsystems under host/ share, and the entry functions
// they call across files.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

#include "stem_kernel.h"
#include "host/runtime.h"
#include "host/sk_internal.h"
#include "kernels/device_set.h"
#include "kernels/launch.h"

namespace sk {

struct DeviceBuffers {
  std::vector<void*> ptrs;
  size_t bytes = 0;  // (SK_HOST_STATS)
  ~DeviceBuffers() { release(); }
  void release() {
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
  }
};

template <class V, class T = typename V::value_type>
hipError_t upload(DeviceBuffers& db, const V& v, const T** out) {
  void* p = nullptr;
  const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) return e;
  db.ptrs.push_back(p);
  db.bytes += bytes;
  if (!v.empty()) e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  *out = static_cast<const T*>(p);
  return e;
}

// Packed host image of a dataset (device_set.h layout).
// vectors whose resize() leaves new elements uninitialised (trivial types):
// the packed arrays are sized once and filled on host threads, which then
// also take the page faults, instead of one thread zero-filling them first
template <class T>
struct NoInitAlloc : std::allocator<T> {
  template <class U>
  struct rebind {
    using other = NoInitAlloc<U>;
  };
  NoInitAlloc() = default;
  template <class U>
  NoInitAlloc(const NoInitAlloc<U>&) noexcept {}
  template <class U>
  void construct(U* p) noexcept {
    ::new ((void*)p) U;
  }
  template <class U, class... A>
  void construct(U* p, A&&... a) {
    ::new ((void*)p) U(std::forward<A>(a)...);
  }
};
template <class T>
using pvec = std::vector<T, NoInitAlloc<T>>;

struct HostPack {
  std::vector<int32_t> ex_nl, ex_node_base, ex_edge_base, ex_bpf_base, ex_lvl_base, ex_nlev,
      ex_len, ex_pos_base, ex_has_w;
  // every profile entry of the example a multiple of 1/256 (BPLA fast path)
  std::vector<uint8_t> ex_dyadic;
  // dyadic and no empty profile column: the string kernel's fast path;
  // every column one residue: its one-hot variant
  std::vector<uint8_t> ex_str_fast, ex_onehot;
  // y examples the register-class stem kernel cannot take (2,048 non-leaf
  // nodes or more -- each class keeps its last slot free --, or a stem edge
  // gap over 1023: its packed 11/11/10-bit records); they go to
  // sk_dag_stem_big_kernel (level-order arrays)
  std::vector<uint8_t> ex_big;
  std::vector<float> ex_nseqs;
  pvec<uint32_t> nd_a, nd_b, nd_c;
  pvec<float> nd_w, nd_nbp;
  pvec<double> nd_P;
  pvec<uint2> ed;
  pvec<uint32_t> bpf_code;
  pvec<float> bpf_p;
  pvec<int32_t> lvl;
  pvec<float4> pos_prof;
  pvec<float> pos_w;
  pvec<uint8_t> pos_chr;
  pvec<float4> pos_lru;
  std::vector<int32_t> ex_nslots, ex_xch_base;
  pvec<sk::XRow> xrow;
  pvec<uint32_t> yn_a, yn_b, yn_c, ye2, ysc;
  pvec<uint4> yrec;
  pvec<float> yn_w, yn_nbp, yn_p0;
  pvec<double> yn_P;
  pvec<int32_t> ycs;
  std::vector<int32_t> ex_ysc_base, ex_nch, ex_ycs_base;
  // the same y records with the equal-length nodes renumbered for the LDS
  // banks (host/pack_sweep.cpp renumber_equal_lengths), at the same offsets, in
  // arrays of their own (the ones above stay the plain stable order by
  // length); empty unless y_renumbered, which also says that the device image
  // holds them as its y records
  pvec<uint32_t> r_yn_a, r_yn_b, r_yn_c, r_ye2, r_ysc;
  pvec<uint4> r_yrec;
  pvec<float> r_yn_w, r_yn_nbp, r_yn_p0;
  pvec<double> r_yn_P;
  bool y_renumbered = false;
  const pvec<uint32_t>& run_ysc() const { return y_renumbered ? r_ysc : ysc; }
  pvec<uint32_t> xr_node, xr_ch;
  // gamma schedule (device_set.h): the x rows without the gamma rows, the
  // gamma rows' K inputs, the dataset's gamma keys and the y gapless flags
  pvec<sk::XRow> xgrow;
  std::vector<uint32_t> gam_key;
  pvec<uint32_t> xg_node, xg_ch, xg_clg, gr_info;
  pvec<float> xg_cpf, gr_pf;
  pvec<double> gr_P;
  std::vector<int32_t> ex_xg_base, ex_nlxg, ex_xgch_base, ex_gr_base, ex_gapless;
  // phi rows (combination rows of the gamma schedule): per child record its
  // weight recipe, the rows' Gamma_{code,len} K inputs, each example's phi
  // components (phi key per type-2 record, in record order), the phi keys
  pvec<uint8_t> xg_cty;
  std::vector<uint32_t> phi_al, phi_g;
  pvec<uint32_t> gra_gidx, gra_row, phk_idx;
  std::vector<int32_t> ex_gra_base, ex_phk_base;
  pvec<uint64_t> ex_phi_bits;  // per example, the phi keys it uses (bitset)
  // the factored gamma schedule (host/pack_shared_sums.cpp): the gamma
  // schedule's rows plus shared-sum combination rows, in arrays of their own
  // (the xg_* arrays stay the plain schedule); xf_gra_row is gra_row in its
  // row numbering, ex_ss_rows / ex_ss_repl count each example's shared-sum
  // rows and the member records they replaced.  Empty unless shared_sums,
  // which also says that the device image holds them as its gamma schedule.
  pvec<sk::XRow> xf_row;
  pvec<uint32_t> xf_node, xf_ch, xf_clg, xf_gra_row;
  pvec<float> xf_cpf;
  pvec<uint8_t> xf_cty;
  std::vector<int32_t> ex_xf_base, ex_nlxf, ex_xfch_base, ex_ss_rows, ex_ss_repl;
  bool shared_sums = false;
  int32_t max_nl = 0, max_edges = 0, max_bpf = 0, max_nlev = 0, max_len = 0, max_slots = 0;
  int32_t max_nch = 0;
  // the gamma schedule the kernel runs
  const pvec<sk::XRow>& run_rows() const { return shared_sums ? xf_row : xgrow; }
  const pvec<uint32_t>& run_ch() const { return shared_sums ? xf_ch : xg_ch; }
  const std::vector<int32_t>& run_base() const { return shared_sums ? ex_xf_base : ex_xg_base; }
  const std::vector<int32_t>& run_nl() const { return shared_sums ? ex_nlxf : ex_nlxg; }
  const std::vector<int32_t>& run_ch_base() const { return shared_sums ? ex_xfch_base : ex_xgch_base; }
};
// Every packed array, named once.  The *_CAT lists are the arrays that
// pack_x / pack_y form per example and pack_dataset concatenates (host/pack.cpp:
// one offset vector, one resize and one copy per name); a list without CAT
// is its CAT part followed by the per-example scalars, bases and key tables.
// sk_dataset_pack_digest and tools/pack_compare.cpp hash the lists in this
// order, which the pinned hashes fix.
// the y records that depend on the numbering of the nodes, under the prefix p
// (none: the plain stable order by length; r_: the renumbered ones)
#define SK_PACK_YREC_ARRAYS(X, p) X(p##yn_a) X(p##yn_b) X(p##yn_c) X(p##ye2) X(p##ysc) X(p##yrec) X(p##yn_w) \
  X(p##yn_nbp) X(p##yn_p0) X(p##yn_P)
#define SK_PACK_Y_CAT_ARRAYS(X) SK_PACK_YREC_ARRAYS(X, ) X(ycs)
#define SK_PACK_Y_ARRAYS(X) SK_PACK_Y_CAT_ARRAYS(X) X(ex_ysc_base) X(ex_nch) X(ex_ycs_base)
#define SK_PACK_YR_ARRAYS(X) SK_PACK_YREC_ARRAYS(X, r_)
#define SK_PACK_X_CAT_ARRAYS(X) X(nd_a) X(nd_b) X(nd_c) X(nd_w) X(nd_nbp) X(nd_P) X(ed) X(bpf_code) X(bpf_p) \
  X(lvl) X(xr_ch) X(xrow) X(xr_node) X(gr_info) X(gr_pf) X(gr_P) X(xg_ch) X(xg_clg) X(xg_cpf) X(xg_cty)     \
  X(phk_idx) X(gra_gidx) X(gra_row) X(xgrow) X(xg_node) X(pos_prof) X(pos_w) X(pos_chr) X(pos_lru)          \
  X(ex_phi_bits)
#define SK_PACK_X_ARRAYS(X) SK_PACK_X_CAT_ARRAYS(X) X(ex_nl) X(ex_node_base) X(ex_edge_base) X(ex_bpf_base) \
  X(ex_lvl_base) X(ex_nlev) X(ex_len) X(ex_pos_base) X(ex_has_w) X(ex_dyadic) X(ex_str_fast) X(ex_onehot)   \
  X(ex_big) X(ex_nseqs) X(ex_nslots) X(ex_xch_base) X(gam_key) X(ex_xg_base) X(ex_nlxg) X(ex_xgch_base)     \
  X(ex_gr_base) X(ex_gapless) X(phi_al) X(phi_g) X(ex_gra_base) X(ex_phk_base)
// the factored schedule's arrays (hashed apart from the lists above)
#define SK_PACK_F_CAT_ARRAYS(X) X(xf_row) X(xf_node) X(xf_ch) X(xf_clg) X(xf_cpf) X(xf_cty) X(xf_gra_row)
#define SK_PACK_F_ARRAYS(X) SK_PACK_F_CAT_ARRAYS(X) X(ex_xf_base) X(ex_nlxf) X(ex_xfch_base) X(ex_ss_rows) \
  X(ex_ss_repl)

// 4-D stem kernel tables of every example of a dataset, resident on the
// device: one set per (device, bp model, loop), built on the first 4-D call
// for it and rebuilt when examples were added since (examples are
// append-only); stem4d_tables.  A call holds its sets through shared_ptrs, and
// a replaced set synchronizes its own device before its buffers are freed,
// so kernels of any context still reading it finish first.
struct Stem4dTables {
  Stem4dTables() = default;
  Stem4dTables(const Stem4dTables&) = delete;
  Stem4dTables& operator=(const Stem4dTables&) = delete;
  ~Stem4dTables() {
    if (device < 0 || buf.ptrs.empty()) return;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) cur = -1;
    if (hipSetDevice(device) == hipSuccess) (void)hipDeviceSynchronize();
    buf.release();
    if (cur >= 0) (void)hipSetDevice(cur);
  }
  DeviceBuffers buf;
  int device = -1, model = -1;
  unsigned loop = 0;
  size_t n_ex = 0;
  const float* bp = nullptr;
  const uint8_t* ch = nullptr;
  std::vector<int64_t> bp_off, ch_off;
  // per example: 0 usable, 1 several rows, 2 no base pairs (bp_model 0);
  // acgu: only A/C/G/U residues (the PairHMM constraints need them)
  std::vector<uint8_t> why, acgu;
};

}  // namespace sk

struct sk_dataset {
  std::vector<sk::Example> ex;
  std::vector<std::string> labels;
  // device image (per device ordinal; one context uploads)
  int device = -1;
  bool uploaded = false;
  sk::DevSet dev;
  sk::DeviceBuffers buf;
  sk::HostPack pack;
  // protein examples (sk_dataset_add_protein): their own packed image, the
  // arrays of sk::LaProtSet and per example whether every column holds one
  // residue kind (the code kernel's pairs); the RNA image above stays empty
  struct ProtPack {
    std::vector<int32_t> ex_len, ex_pos_base;
    std::vector<uint8_t> ex_coded, code;
    std::vector<float> prof;
  } ppack;
  sk::LaProtSet pdev;
  // palindrome examples (sk_dataset_add_palindromes): the arrays of
  // sk::SimpalSet, every example's entries one contiguous run
  struct PalPack {
    std::vector<int32_t> ex_off, dist;
    std::vector<uint64_t> key;
    std::vector<float> w;
  } spack;
  sk::SimpalSet sdev;
  std::string err;
  // x-role leaf-column closed forms (sk_prep_kernel) for one loop_gap: they
  // depend only on the dataset (immutable once uploaded) and loop_gap
  double* prep = nullptr;
  double prep_loop_gap = -1.0;
  // 4-D tables per (device, bp model, loop), at most kS4Sets (oldest dropped)
  std::mutex s4_mu;
  std::vector<std::shared_ptr<sk::Stem4dTables>> s4;
};

namespace sk {

constexpr size_t kS4Sets = 4;

// A dataset is RNA, protein or palindrome, decided by its first example.
enum { kSortRna = 0, kSortProtein = 1, kSortPal = 2 };
inline int ex_sort(const Example& X) { return X.pal ? kSortPal : X.protein ? kSortProtein : kSortRna; }
inline bool ds_protein(const sk_dataset* ds) { return !ds->ex.empty() && ds->ex[0].protein; }
inline bool ds_pal(const sk_dataset* ds) { return !ds->ex.empty() && ds->ex[0].pal; }
// appending an example of another sort: refused (the message in ds->err)
inline bool ds_mixes(sk_dataset* ds, int sort) {
  if (ds->ex.empty() || ex_sort(ds->ex[0]) == sort) return false;
  static const char* const name[3] = {"RNA", "protein", "palindrome"};
  static const char* const art[3] = {"an", "a", "a"};
  ds->err = std::string(name[sort]) + " example added to " + art[ex_sort(ds->ex[0])] + " " +
            name[ex_sort(ds->ex[0])] + " dataset";
  return true;
}
// a palindrome dataset holds one seed_length (the reference asserts equal key
// lengths, simpal/simpal.cpp:272)
inline bool pal_seed_differs(sk_dataset* ds, int32_t seed_length) {
  if (!ds_pal(ds) || ds->ex[0].pal_seed == seed_length) return false;
  ds->err = "palindrome example of another seed_length than the dataset's";
  return true;
}
struct Stem4dBatch {
  sk::Stem4dPair* pairs = nullptr;
  int2* items = nullptr;
  int32_t* band = nullptr;  // c_low | c_high (cap_band each)
  size_t cap_pairs = 0, cap_items = 0, cap_band = 0;
};

}  // namespace sk

struct sk_context {
  sk::Stem4dBatch s4d;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int n_cu = 0;
  std::string err;
  // reusable device buffers
  double* scratch = nullptr;
  size_t scratch_bytes = 0;
  void* work = nullptr;
  size_t work_bytes = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
  // side stream: the string kernel of a stem+string kind runs beside the
  // persistent stem launches and fills the CUs their tails free
  hipStream_t side = nullptr;
  hipEvent_t evf = nullptr, evj = nullptr;
  // second class stream: DAG stem register classes alternate between the
  // main stream and this one, so a class's fill overlaps the previous one's
  // tail
  hipStream_t cls = nullptr;
  hipEvent_t evk = nullptr, evx = nullptr;
  // a fourth stream: the 4-D kernel's span launches run in parts on all four
  hipStream_t aux = nullptr;
  hipEvent_t eva = nullptr;
  // Timing of a compute call: its span events (ev0..ev3 are the current
  // set's) and per-launch events of the dominant kernel (sk_last_launch_ms: a
  // start and an end event around each launch on the launch's own stream).
  // Synchronous calls use set 0 and are resolved before they return; with
  // sk_set_async the sets rotate through a ring and a call returns once its
  // work is enqueued: its set stays pending until sk_sync_timing, or until
  // the ring comes round to it, and is then added to the acc_* totals.
  struct TSet {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> lev;
    size_t lev_used = 0;
    bool pending = false, stem = false, str = false;
    double cells = 0.0;
    int32_t launches = 0;
  };
  static constexpr int kTSets = 4;
  TSet tset[kTSets];
  int tk = 0;
  bool async = false;
  double acc_stem_ms = 0.0, acc_str_ms = 0.0, acc_cells = 0.0, acc_launch_ms = 0.0;
  int32_t acc_launch_n = 0, acc_launches = 0;
  // pinned staging of an asynchronous call's host-to-device uploads (the
  // host buffers die when the call returns; pageable copies would wait for
  // the stream): one ring slot per call parity, reused once its copies are
  // done (its event)
  struct Stage {
    std::vector<std::pair<char*, size_t>> blocks;
    size_t blk = 0, off = 0;
    hipEvent_t ev = nullptr;
    bool recorded = false;
    // device copy of a call's inputs uploaded on the copy stream (up_reserve)
    char* dbuf = nullptr;
    size_t dcap = 0;
    hipEvent_t uev = nullptr;
  };
  Stage stage[2];
  hipStream_t cps = nullptr;  // copy stream of the asynchronous uploads
  uint64_t ncalls = 0;
  double last_launch_ms_sum = 0.0;
  int32_t last_launch_n = 0;
  double last_stem_ms = 0.0, last_str_ms = 0.0, last_cells = 0.0;
  int32_t last_launches = 0;
  // kernel instantiations the last compute call launched (sk_last_classes):
  // bit MAXK/4 per DAG stem register class; bit log2(CPL) (+4 when banded)
  // per 4-D stem class
  uint32_t last_stem_classes = 0, last_s4d_classes = 0;
  int32_t last_gamma_shared = 0;  // class launches of the last call that read shared Gamma (and Phi) tables
  uint32_t last_la_protein = 0;   // protein LA kernels of the last call: 1 code, 2 profile
  // string kernels of the last call (sk_last_string): one-hot fast, dyadic fast, general
  int64_t last_str_pairs[3] = {0, 0, 0};
  int32_t last_str_waves[3] = {0, 0, 0};  // waves per workgroup of each launch
  uint32_t last_la_protein_grad = 0;  // protein LA gradient kernels of the last gradient call: 1 code, 2 profile
  uint32_t last_stem_grad = 0;  // stem gradient kernels of the last gradient call: 1 Su, 2 Si
  // RCCL communicator of sk_comm_init (ncclComm_t, csrc/host/shard.cpp)
  void* comm = nullptr;
};

namespace sk {

// Host thread pools: f(t) for t = 1..n-1 on new threads, f(0) on the calling
// thread; a slice whose thread cannot be created (std::system_error) runs on
// the calling thread too, so a pool never escapes through the C ABI.  The
// no-index form is for workers that share an atomic cursor.
template <class F>
void run_slices(int n, F&& f) {
  std::vector<std::thread> th;
  std::vector<int> here;
  for (int t = 1; t < n; ++t) {
    try {
      th.emplace_back(f, t);
    } catch (const std::system_error&) {
      here.push_back(t);
    }
  }
  f(0);
  for (int t : here) f(t);
  for (auto& x : th) x.join();
}
// host threads of a call's planning passes (the box gives a job 16)
inline int plan_threads(int want) {
  return std::max(1, std::min({want, 16, (int)std::max(1u, std::thread::hardware_concurrency())}));
}
template <class F>
void run_pool(int n, F&& work) {
  std::vector<std::thread> th;
  for (int t = 1; t < n; ++t) {
    try {
      th.emplace_back(work);
    } catch (const std::system_error&) {
      break;  // the calling thread's share drains the cursor
    }
  }
  work();
  for (auto& x : th) x.join();
}

inline int fail(sk_context* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

#define SK_HIP(ctx, expr)                                                              \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return sk::fail((ctx), SK_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// ------------------------------------------------------------ parameters
inline bool kind_is_bpla(int k) { return k >= SK_BPLA && k <= SK_LA_SW; }
inline bool kind_is_aa(int k) { return k == SK_AA_LA || k == SK_AA_LA_SW; }
inline bool kind_has_stem(int k) {
  return k != SK_SU_STR && k != SK_SI_STR && k != SK_NAIVE_STR && !kind_is_bpla(k) &&
         k != SK_STEM4D && !kind_is_aa(k) && k != SK_SIMPAL;
}
inline bool kind_has_str(int k) {
  return k == SK_SU_STR || k == SK_SI_STR || k == SK_SU_STEM_STR || k == SK_SI_STEM_STR ||
         k == SK_LSU_STEM_STR || k == SK_NAIVE_STR;
}
inline bool kind_subst(int k) {  // RIBOSUM (Su*) vs match/mismatch (Si*)
  return k == SK_SU_STEM || k == SK_SU_STR || k == SK_SU_STEM_STR || k == SK_LSU_STEM ||
         k == SK_LSU_STEM_STR;
}
inline int32_t combine_mode(int k) {
  switch (k) {
    case SK_SU_STEM:
    case SK_SI_STEM: return sk::kCombineStem;
    case SK_SU_STR:
    case SK_SI_STR:
    case SK_NAIVE_STR: return sk::kCombineStr;
    case SK_SU_STEM_STR:
    case SK_SI_STEM_STR: return sk::kCombineAdd;
    case SK_LSU_STEM: return sk::kCombineLogStem;
    default: return sk::kCombineLogAdd;
  }
}

inline std::vector<double> gap_powers(double g, int n) {
  // SimpleEdgeScore::initialize (score_table.cpp:60-77): g[k] = g[k-1]*gap
  std::vector<double> v(std::max(n, 1));
  v[0] = 1.0;
  for (int k = 1; k < n; ++k) v[k] = v[k - 1] * g;
  return v;
}

// a bump allocator over a context's work buffer
struct Arena {
  char* base;
  size_t off = 0, cap;
  template <class T>
  T* take(size_t n) {
    off = (off + 255) & ~size_t(255);
    T* p = reinterpret_cast<T*>(base + off);
    off += n * sizeof(T);
    return p;
  }
};

// ------------------------------------------------------------ across files
// the packer (host/pack.cpp, over the per-example passes that
// host/pack_internal.h declares; tools/pack_compare.cpp times it) and one
// position's BPLA weights as it forms them (sk_dataset_bpla_weights)
int pack_dataset(sk_dataset* ds, std::string& err, const std::function<void()>* after_x = nullptr);
float4 bpla_weight(const Example& X, int i);
// the planners behind sk_api.cpp's run_pairs, one per family of kinds: the
// DAG stem and string kinds (host/pairs_dag.cpp), BPLA (host/pairs_bpla.cpp),
// protein LA (host/pairs_la_protein.cpp), palindromes (host/pairs_simpal.cpp)
// and the 4-D stem kernel (host/pairs_stem4d.cpp)
int run_dag_pairs(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
                  const int32_t* x, const int32_t* y, int64_t n, double* out_dev);
int run_bpla(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
             const int32_t* x, const int32_t* y, int64_t n, double* out_dev);
int run_la_protein(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
                   const int32_t* x, const int32_t* y, int64_t n, double* out_dev);
int run_simpal(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
               const int32_t* x, const int32_t* y, int64_t n, double* out_dev);
int run_stem4d(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
               const int32_t* x, const int32_t* y, int64_t n, double* out_dev);
// the BPLA gradient driver behind sk_bpla_gradients (host/pairs_bpla.cpp)
int bpla_gradients(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
                   const int32_t* x, const int32_t* y, int64_t n, double* value, double* grad);
// the planner of the stem gradient kernels behind sk_stem_gradients
// (host/pairs_stem_grad.cpp): the stem part Ks and d/d(loop_gap, beta, stack,
// covar) of checked pairs, to host buffers (synchronous)
int stem_gradients_gpu(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
                       const int32_t* x, const int32_t* y, int64_t n, double* value, double* grad);
// example builders of host/dataset.cpp that the GPU folds' adders
// (host/fold_gpu.cpp), the byte format (host/dataset_io.cpp) and sk_api.cpp
// use.  kAaMaxRows: protein examples of this many rows or more are refused
// (below it every float product and sum of LAScore's weight n is an exact
// integer, < 2^24)
constexpr int kAaMaxRows = 4096;
int char2aa(int c);
int pal_args(size_t n, int32_t seed_length, int32_t min_loop, int32_t max_dist, std::string* err);
void build_palindromes(Example& ex, const std::string& seq, const double* bpp, int32_t s, int32_t min_loop,
                       int32_t max_dist);
std::string lower(const char* s);
int add_examples_threaded(sk_dataset* ds, int32_t n, int32_t n_rows, const char* const* rows,
                          const double* const* bpp_rows, const char* const* labels, float th,
                          int use_bp, int32_t n_threads, bool consensus = false);

}  // namespace sk
