// C ABI of the stem-kernel engine (include/stem_kernel.h): the front door.
//
// The pair calls -- their argument checks and the dispatch by kernel kind to
// the planners under host/ -- and the entry points built on them (Gram, test
// rows and matrices, diagonal), which replace KernelMatrix::calculate's
// per-pair loop (common/kernel_matrix.cpp:42-56, 485-575); the default
// parameters and the one-line accessors.  The context, the packer, the
// datasets, the byte format and the GPU folds each have a file under host/.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "host/runtime_types.h"
#include "ribosum85_60.inc"
#include "blosum62.inc"

namespace sk {
namespace {

// Core: out_dev[k] = K(xset[x[k]], yset[y[k]]) (device buffer), async.
int run_pairs(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
              const int32_t* x, const int32_t* y, int64_t n, double* out_dev) {
  if (!ctx || !kp) return fail(ctx, SK_ERR_INVALID, "null argument");
  int rc = check_set(ctx, xs_);
  if (rc) return rc;
  rc = check_set(ctx, ys_);
  if (rc) return rc;
  if (n < 0) return fail(ctx, SK_ERR_INVALID, "negative pair count");
  if (kp->kind < SK_SU_STEM || kp->kind > SK_SIMPAL)
    return fail(ctx, SK_ERR_UNSUPPORTED, "unknown kernel kind");
  // palindrome datasets and SK_SIMPAL go together, and with nothing else
  if (ds_pal(xs_) != ds_pal(ys_) && !xs_->ex.empty() && !ys_->ex.empty())
    return fail(ctx, SK_ERR_INVALID, "a palindrome dataset paired with a dataset of another sort");
  if (kp->kind == SK_SIMPAL && !(ds_pal(xs_) && ds_pal(ys_)) && n > 0)
    return fail(ctx, SK_ERR_INVALID, "the palindrome kernel kind (SK_SIMPAL) needs palindrome datasets (sk_dataset_add_palindromes)");
  if (kp->kind != SK_SIMPAL && (ds_pal(xs_) || ds_pal(ys_)))
    return fail(ctx, SK_ERR_INVALID, "a kernel kind other than SK_SIMPAL on a palindrome dataset");
  // no silent reinterpretation of one alphabet as the other
  if (ds_protein(xs_) != ds_protein(ys_) && !xs_->ex.empty() && !ys_->ex.empty())
    return fail(ctx, SK_ERR_INVALID, "a protein dataset paired with an RNA dataset");
  if (kind_is_aa(kp->kind) && !(ds_protein(xs_) && ds_protein(ys_)) && n > 0)
    return fail(ctx, SK_ERR_INVALID, "an amino-acid kernel kind (SK_AA_LA*) needs protein datasets, these hold RNA examples");
  if (!kind_is_aa(kp->kind) && (ds_protein(xs_) || ds_protein(ys_)))
    return fail(ctx, SK_ERR_INVALID, "an RNA kernel kind on a protein dataset (use SK_AA_LA or SK_AA_LA_SW)");
  ctx->last_stem_ms = ctx->last_str_ms = ctx->last_cells = 0.0;
  ctx->last_launches = 0;
  sk::lev_reset(ctx);
  ctx->last_stem_classes = ctx->last_s4d_classes = 0;
  ctx->last_gamma_shared = 0;
  ctx->last_la_protein = 0;
  for (int k = 0; k < 3; ++k) ctx->last_str_pairs[k] = ctx->last_str_waves[k] = 0;
  if (n == 0) return SK_OK;
  const int nx = (int)xs_->ex.size(), ny = (int)ys_->ex.size();
  for (int64_t k = 0; k < n; ++k)
    if (x[k] < 0 || x[k] >= nx || y[k] < 0 || y[k] >= ny)
      return fail(ctx, SK_ERR_RANGE, "pair index out of range");
  SK_HIP(ctx, sk::call_begin(ctx));
  if (kind_is_bpla(kp->kind)) return run_bpla(ctx, xs_, ys_, kp, x, y, n, out_dev);
  if (kind_is_aa(kp->kind)) return run_la_protein(ctx, xs_, ys_, kp, x, y, n, out_dev);
  if (kp->kind == SK_SIMPAL) return run_simpal(ctx, xs_, ys_, kp, x, y, n, out_dev);
  if (kp->kind == SK_STEM4D) {
    // synchronous batches (each waits for its spans): its totals are final
    rc = run_stem4d(ctx, xs_, ys_, kp, x, y, n, out_dev);
    if (rc == SK_OK && ctx->async) {
      ctx->acc_stem_ms += ctx->last_stem_ms;
      ctx->acc_cells += ctx->last_cells;
      ctx->acc_launches += ctx->last_launches;
      ctx->acc_launch_ms += ctx->last_launch_ms_sum;
      ctx->acc_launch_n += ctx->last_launch_n;
    }
    return rc;
  }

  return run_dag_pairs(ctx, xs_, ys_, kp, x, y, n, out_dev);  // the DAG stem and string kinds (host/pairs_dag.cpp)
}

int pairs_host(sk_context* ctx, sk_dataset* xs_, sk_dataset* ys_, const sk_kernel_params* kp,
               const int32_t* x, const int32_t* y, int64_t n, double* out) {
  if (n == 0) return SK_OK;
  double* d = nullptr;
  SK_HIP(ctx, hipMalloc(&d, (size_t)n * sizeof(double)));
  int rc = run_pairs(ctx, xs_, ys_, kp, x, y, n, d);
  if (rc == SK_OK) {
    // the results are on the context's stream (an asynchronous call has not
    // waited for them): read them in its order
    hipError_t e = hipMemcpyAsync(out, d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = fail(ctx, SK_ERR_HIP, hipGetErrorString(e));
  }
  (void)hipFree(d);
  return rc;
}

}  // namespace
}  // namespace sk

extern "C" {

void sk_kernel_params_default(sk_kernel_params* p, int32_t kind) {
  if (!p) return;
  p->kind = kind;
  p->len_band = 10;
  p->beta = 0.3;
  p->loop_gap = 0.2;
  p->stack = 1.3;
  p->covar = 0.8;
  p->alpha = 0.2;
  p->gap = 0.8;
  p->match = 1.0;
  p->mismatch = 0.8;
  // bpla_kernel/main.cpp:20-26 (float table), 68-76 (float options)
  static const float kBplaTable[16] = {5.846613f,  -1.860000f, -1.460000f, -1.390000f,
                                       -1.860000f, 4.786613f,  -2.480000f, -1.050000f,
                                       -1.460000f, -2.480000f, 4.656613f,  -1.740000f,
                                       -1.390000f, -1.050000f, -1.740000f, 5.276613f};
  for (int k = 0; k < 16; ++k) p->score_table[k] = (double)kBplaTable[k];
  p->ext = (double)-0.75f;
  // stem_kernel/main.cpp:40-60 (float options; bp_bound default of -p)
  p->subst = (double)0.5f;
  p->bp_bound = 0.0;
  p->bp_model = 0;
  p->loop = 3;
  p->ali_bound = 0.0;
  p->ali_zerop_fixed = 0;
  if (kind == SK_STEM4D) {
    p->gap = (double)0.8f;
    p->stack = (double)1.0f;
    p->len_band = 0;
  }
  if (kind >= SK_BPLA && kind <= SK_LA_SW) {
    p->gap = (double)-8.0f;
    p->alpha = (double)4.5f;
    p->beta = (double)0.11f;
  }
  // la_main.cpp:21-46 (BLOSUM62), 87-90 (float options)
  for (int k = 0; k < 529; ++k) p->aa_score_table[k] = (double)SK_BLOSUM62[k];
  if (kind == SK_AA_LA || kind == SK_AA_LA_SW) {
    p->gap = (double)-10.0f;
    p->ext = (double)-1.0f;
    p->beta = (double)0.11f;
  }
  // simpal/simpal.cpp:316, 335: tolerance 1, carried by the mismatch field
  if (kind == SK_SIMPAL) p->mismatch = 1.0;
}

int sk_pairs_device(sk_context* ctx, sk_dataset* ds, const sk_kernel_params* kp, const int32_t* x,
                    const int32_t* y, int64_t n_pairs, double* out_dev) {
  return sk::run_pairs(ctx, ds, ds, kp, x, y, n_pairs, out_dev);
}

int sk_bpla_gradients(sk_context* ctx, sk_dataset* xs, sk_dataset* ys, const sk_kernel_params* kp,
                      const int32_t* x, const int32_t* y, int64_t n_pairs, double* value,
                      double* grad) {
  return sk::bpla_gradients(ctx, xs, ys, kp, x, y, n_pairs, value, grad);
}

int sk_pairs(sk_context* ctx, sk_dataset* ds, const sk_kernel_params* kp, const int32_t* x,
             const int32_t* y, int64_t n_pairs, double* out) {
  return sk::pairs_host(ctx, ds, ds, kp, x, y, n_pairs, out);
}

int sk_gram(sk_context* ctx, sk_dataset* ds, const sk_kernel_params* kp, int normalize,
            double* out) {
  if (!ctx || !ds || !kp || !out) return sk::fail(ctx, SK_ERR_INVALID, "null argument");
  const int n = (int)ds->ex.size();
  std::vector<int32_t> xi, yi;
  xi.reserve((size_t)n * (n + 1) / 2);
  yi.reserve((size_t)n * (n + 1) / 2);
  // the reference's cell order (kernel_matrix.cpp:44-55): i outer, j >= i
  for (int i = 0; i < n; ++i)
    for (int j = i; j < n; ++j) {
      xi.push_back(i);
      yi.push_back(j);
    }
  std::vector<double> v(std::max<size_t>(xi.size(), 1));
  int rc = sk::pairs_host(ctx, ds, ds, kp, xi.data(), yi.data(), (int64_t)xi.size(), v.data());
  if (rc) return rc;
  // mirror + normalise (kernel_matrix.cpp:560-571): the one-rank case of the
  // sharded assembly (csrc/host/shard.cpp), so both give the same bits
  return sk_shard_assemble(n, 1, v.data(), (int64_t)v.size(), normalize, out);
}

int sk_test_row(sk_context* ctx, sk_dataset* test, int t, sk_dataset* train,
                const int32_t* sv_index, int32_t n_sv, const sk_kernel_params* kp, double* out,
                double* self) {
  if (!ctx || !test || !train || !kp || !out) return sk::fail(ctx, SK_ERR_INVALID, "null argument");
  if (t < 0 || t >= (int)test->ex.size()) return sk::fail(ctx, SK_ERR_RANGE, "test index");
  const int ntr = (int)train->ex.size();
  std::vector<int32_t> xi, yi;
  if (sv_index) {
    for (int32_t k = 0; k < n_sv; ++k) {
      if (sv_index[k] < 0 || sv_index[k] >= ntr) return sk::fail(ctx, SK_ERR_RANGE, "sv index");
      xi.push_back(sv_index[k]);
    }
  } else {
    for (int i = 0; i < ntr; ++i) xi.push_back(i);
  }
  yi.assign(xi.size(), t);
  std::vector<double> v(xi.size());
  // kernel_(train_[i].second, data_.second): x = train, y = test
  int rc = sk::pairs_host(ctx, train, test, kp, xi.data(), yi.data(), (int64_t)xi.size(), v.data());
  if (rc) return rc;
  for (size_t k = 0; k < xi.size(); ++k) out[xi[k]] = v[k];
  if (self) {
    const int32_t a = t;
    rc = sk::pairs_host(ctx, test, test, kp, &a, &a, 1, self);
    if (rc) return rc;
  }
  return SK_OK;
}

int sk_diagonal(sk_context* ctx, sk_dataset* ds, const int32_t* sv_index, int32_t n_sv,
                const sk_kernel_params* kp, double* out) {
  if (!ctx || !ds || !kp || !out) return sk::fail(ctx, SK_ERR_INVALID, "null argument");
  const int n = (int)ds->ex.size();
  std::vector<int32_t> xi;
  if (sv_index) {
    for (int32_t k = 0; k < n_sv; ++k) {
      if (sv_index[k] < 0 || sv_index[k] >= n) return sk::fail(ctx, SK_ERR_RANGE, "sv index");
      xi.push_back(sv_index[k]);
    }
  } else {
    for (int i = 0; i < n; ++i) xi.push_back(i);
  }
  std::vector<double> v(xi.size());
  int rc = sk::pairs_host(ctx, ds, ds, kp, xi.data(), xi.data(), (int64_t)xi.size(), v.data());
  if (rc) return rc;
  for (size_t k = 0; k < xi.size(); ++k) out[xi[k]] = v[k];
  return SK_OK;
}

int sk_test_matrix(sk_context* ctx, sk_dataset* test, sk_dataset* train,
                   const sk_kernel_params* kp, int norm_test, int normalize, double* out,
                   double* self_out) {
  if (!ctx || !test || !train || !kp || !out) return sk::fail(ctx, SK_ERR_INVALID, "null argument");
  const int nt = (int)test->ex.size(), ntr = (int)train->ex.size();
  std::vector<int32_t> xi, yi;
  for (int i = 0; i < nt; ++i)
    for (int j = 0; j < ntr; ++j) {
      xi.push_back(j);
      yi.push_back(i);
    }
  int rc = sk::pairs_host(ctx, train, test, kp, xi.data(), yi.data(), (int64_t)xi.size(), out);
  if (rc) return rc;
  std::vector<double> self(nt, 0.0);
  if (norm_test || normalize) {
    std::vector<int32_t> ti(nt);
    std::iota(ti.begin(), ti.end(), 0);
    rc = sk::pairs_host(ctx, test, test, kp, ti.data(), ti.data(), nt, self.data());
    if (rc) return rc;
    if (self_out) std::copy(self.begin(), self.end(), self_out);
  }
  if (normalize) {
    std::vector<double> diag(ntr);
    rc = sk_diagonal(ctx, train, nullptr, 0, kp, diag.data());
    if (rc) return rc;
    for (int i = 0; i < nt; ++i)
      for (int j = 0; j < ntr; ++j) out[(size_t)i * ntr + j] /= std::sqrt(self[i] * diag[j]);
  }
  return SK_OK;
}

int sk_format_libsvm(const double* m, int32_t rows, int32_t cols, const char* const* labels,
                     char* buf, size_t buf_size, size_t* needed) {
  if ((!m && rows * cols) || rows < 0 || cols < 0) return SK_ERR_INVALID;
  // KernelMatrix::print (kernel_matrix.cpp:756-770): ostream defaults
  std::ostringstream os;
  for (int32_t i = 0; i < rows; ++i) {
    os << (labels && labels[i] ? labels[i] : "") << " 0:" << (i + 1) << " ";
    for (int32_t j = 0; j < cols; ++j) os << (j + 1) << ":" << m[(size_t)i * cols + j] << " ";
    os << "\n";
  }
  const std::string s = os.str();
  if (needed) *needed = s.size() + 1;
  if (buf) {
    if (buf_size < s.size() + 1) return SK_ERR_RANGE;
    std::memcpy(buf, s.c_str(), s.size() + 1);
  }
  return SK_OK;
}

int sk_fold_synthetic(const char* seq, int32_t n, int32_t no_gu, double* out) {
  if (!seq || n < 0 || (!out && n > 1)) return SK_ERR_INVALID;
  try {
    sk::fold_nussinov(seq, n, no_gu != 0, out);
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
  return SK_OK;
}

int sk_char2aa(int c) { return sk::char2aa(c); }

int sk_random_sequences(uint64_t* state, int32_t n_seqs, int32_t len, char* out) {
  if (!state || !out || n_seqs < 0 || len < 0) return SK_ERR_INVALID;
  for (int32_t s = 0; s < n_seqs; ++s) sk::random_sequence(*state, len, out + (size_t)s * (len + 1));
  return SK_OK;
}

void sk_ribosum_tables(float* s16, float* p256) {
  if (s16) std::memcpy(s16, SK_RIBOSUM_S, sizeof(SK_RIBOSUM_S));
  if (p256) std::memcpy(p256, SK_RIBOSUM_P, sizeof(SK_RIBOSUM_P));
}

int sk_char2rna(int c) { return sk::char2rna(c); }

int sk_experiments(void) {
#ifdef SK_EXPERIMENTS
  return 1;
#else
  return 0;
#endif
}

}  // extern "C"
