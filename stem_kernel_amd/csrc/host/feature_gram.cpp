// Feature sets (libsvm feature files) and the host path of the feature-vector
// Grams: RBFKernel / PolyKernel / SigmoidKernel ::calculate_matrix and
// read_data of the reference's optimizer (optimizer/rbf_kernel.cpp,
// poly_kernel.cpp, sigmoid_kernel.cpp).  The arithmetic contract -- the dense
// in-order dot and the epilogue, operation for operation -- is in
// feature_gram.h; this file is compiled with -ffp-contract=off and is what the
// GPU path (csrc/kernels/feature_gram.hip) is compared with.
#include "feature_gram.h"

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <system_error>
#include <thread>

#include "stem_kernel.h"

namespace sk {

namespace {
thread_local std::string g_feat_err;

bool is_blank(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

// the sorted union of the indices in use; what the rows' entries are checked for
int finish(sk_features* fs, std::string& err, const char* who) {
  const int64_t nnz = (int64_t)fs->index.size();
  for (int32_t i = 0; i < fs->n; ++i) {
    const int64_t a = fs->row_ptr[i], b = fs->row_ptr[i + 1];
    if (a > b || a < 0 || b > nnz) {
      err = std::string(who) + ": row_ptr is not ascending within [0, nnz]";
      return SK_ERR_INVALID;
    }
    for (int64_t k = a; k < b; ++k) {
      if (fs->index[k] < 0 || (k > a && fs->index[k] <= fs->index[k - 1])) {
        err = std::string(who) + ": example " + std::to_string(i) + ": indices must be >= 0 and strictly ascending";
        return SK_ERR_INVALID;
      }
      if (!std::isfinite(fs->value[k])) {
        err = std::string(who) + ": example " + std::to_string(i) + ": a value is not finite";
        return SK_ERR_INVALID;
      }
    }
  }
  fs->cols = fs->index;
  std::sort(fs->cols.begin(), fs->cols.end());
  fs->cols.erase(std::unique(fs->cols.begin(), fs->cols.end()), fs->cols.end());
  return SK_OK;
}

// read_data (rbf_kernel.cpp:69-104), with the stricter cases of the header
int parse_text(const char* text, size_t len, sk_features* fs, std::string& err) {
  fs->row_ptr.push_back(0);
  size_t pos = 0;
  int64_t line_no = 0;
  std::string tok;
  while (pos < len) {  // std::getline: a last line without '\n' counts, an empty rest does not
    const char* nl = static_cast<const char*>(std::memchr(text + pos, '\n', len - pos));
    const size_t end = nl ? (size_t)(nl - text) : len;
    ++line_no;
    const std::string where = "line " + std::to_string(line_no) + ": ";
    size_t p = pos;
    bool first = true;
    int32_t last = -1;
    int32_t label = 0;  // a blank line: atoi("") = 0, no features
    while (true) {
      while (p < end && is_blank(text[p])) ++p;
      if (p >= end) break;
      size_t q = p;
      while (q < end && !is_blank(text[q])) ++q;
      tok.assign(text + p, q - p);
      p = q;
      if (first) {
        first = false;
        const long v = std::strtol(tok.c_str(), nullptr, 10);  // atoi
        label = (int32_t)std::max<long>(INT_MIN, std::min<long>(INT_MAX, v));
        continue;
      }
      const size_t colon = tok.find(':');
      if (colon == std::string::npos) {
        err = where + "token '" + tok + "' has no ':'";
        return SK_ERR_INVALID;
      }
      char* e = nullptr;
      errno = 0;
      const long idx = std::strtol(tok.c_str(), &e, 10);
      if (e == tok.c_str() || (size_t)(e - tok.c_str()) != colon || errno == ERANGE || idx > INT_MAX) {
        err = where + "token '" + tok + "': the index is not an integer";
        return SK_ERR_INVALID;
      }
      if (idx < 0) {
        err = where + "index " + std::to_string(idx) + " is negative";
        return SK_ERR_INVALID;
      }
      if (idx <= last) {
        err = where + "index " + std::to_string(idx) + " after " + std::to_string(last) +
              ": indices must be strictly ascending";
        return SK_ERR_INVALID;
      }
      const char* vs = tok.c_str() + colon + 1;
      const double val = std::strtod(vs, &e);
      if (e == vs || *e != '\0') {
        err = where + "token '" + tok + "': the value is not a number";
        return SK_ERR_INVALID;
      }
      if (!std::isfinite(val)) {
        err = where + "token '" + tok + "': the value is not finite";
        return SK_ERR_INVALID;
      }
      last = (int32_t)idx;
      fs->index.push_back((int32_t)idx);
      fs->value.push_back(val);
    }
    fs->labels.push_back(label);
    fs->row_ptr.push_back((int64_t)fs->index.size());
    if (fs->labels.size() > (size_t)INT32_MAX - 1) {
      err = "over 2^31 examples";
      return SK_ERR_UNSUPPORTED;
    }
    pos = end + 1;
  }
  fs->n = (int32_t)fs->labels.size();
  return finish(fs, err, "sk_features_parse");
}

template <class F>
void on_threads(int n_threads, int64_t n_items, F&& f) {
  int nt = n_threads ? n_threads : (int)std::max(1u, std::thread::hardware_concurrency());
  nt = (int)std::max<int64_t>(1, std::min<int64_t>(nt, n_items));
  std::atomic<int64_t> cursor{0};
  auto work = [&] {
    for (int64_t i; (i = cursor.fetch_add(1)) < n_items;) f(i);
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t) {
    try {
      th.emplace_back(work);
    } catch (const std::system_error&) {
      break;  // the calling thread drains the cursor
    }
  }
  work();
  for (auto& x : th) x.join();
}

// rows [i0, i1) of D = X Y^T, each entry the in-order sum from +0, multiply
// then add; sym: only j >= i, mirrored.  kJ entries of a row advance together
// (independent chains; the order within each entry is untouched).
constexpr int kJ = 8;
void dot_row(const double* X, const double* Y, int64_t i, int64_t ny, int64_t d, bool sym, double* D, int64_t ld) {
  const double* x = X + i * d;
  for (int64_t j0 = sym ? i : 0; j0 < ny; j0 += kJ) {
    const int nb = (int)std::min<int64_t>(kJ, ny - j0);
    double acc[kJ] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (nb == kJ) {
      const double* y = Y + j0 * d;
      for (int64_t k = 0; k < d; ++k) {
        const double xk = x[k];
        for (int b = 0; b < kJ; ++b) acc[b] += xk * y[b * d + k];
      }
    } else {
      for (int b = 0; b < nb; ++b) {
        const double* y = Y + (j0 + b) * d;
        double s = 0;
        for (int64_t k = 0; k < d; ++k) s += x[k] * y[k];
        acc[b] = s;
      }
    }
    for (int b = 0; b < nb; ++b) {
      D[i * ld + j0 + b] = acc[b];
      if (sym) D[(j0 + b) * ld + i] = acc[b];
    }
  }
}

void dots_host(const sk_features* xs, const sk_features* ys, int n_threads, double* D, std::vector<double>* nx,
               std::vector<double>* ny) {
  const std::vector<int32_t> cols = feat_columns(xs, ys);
  const int64_t d = (int64_t)cols.size();
  std::vector<double> X((size_t)std::max<int64_t>(1, xs->n * d)), Yv;
  feat_dense(xs, cols, X.data());
  const double* Y = X.data();
  if (ys) {
    Yv.resize((size_t)std::max<int64_t>(1, ys->n * d));
    feat_dense(ys, cols, Yv.data());
    Y = Yv.data();
  }
  const int64_t n_y = ys ? ys->n : xs->n;
  on_threads(n_threads, xs->n, [&](int64_t i) { dot_row(X.data(), Y, i, n_y, d, !ys, D, n_y); });
  auto norms = [&](const double* A, int64_t n, std::vector<double>& out) {
    out.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      double s = 0;
      for (int64_t k = 0; k < d; ++k) s += A[i * d + k] * A[i * d + k];
      out[i] = s;
    }
  };
  if (nx && ys) norms(X.data(), xs->n, *nx);
  if (ny && ys) norms(Y, ys->n, *ny);
}

template <int KIND>
void apply_host(const double* D, int64_t nx, int64_t ny, const double* dx, const double* dy, bool sym, int degree,
                const double* params, int n_threads, double* K, double* G) {
  const double p0 = params[0], p1 = KIND == kFeatRbf ? 0.0 : params[1];
  const int64_t nn = nx * ny;
  on_threads(n_threads, nx, [&](int64_t i) {
    for (int64_t j = sym ? i : 0; j < ny; ++j) {
      double k, g0, g1 = 0;
      const double dii = sym ? D[i * ny + i] : dx[i], djj = sym ? D[j * ny + j] : dy[j];
      feat_entry<KIND>(D[i * ny + j], dii, djj, degree, p0, p1, k, g0, g1);
      K[i * ny + j] = k;
      if (sym) K[j * ny + i] = k;
      if (G) {
        G[i * ny + j] = g0;
        if (sym) G[j * ny + i] = g0;
        if (KIND != kFeatRbf) {
          G[nn + i * ny + j] = g1;
          if (sym) G[nn + j * ny + i] = g1;
        }
      }
    }
  });
}

int gram_host(const char* who, const sk_features* xs, const sk_features* ys, int kind, int degree,
              const double* params, int n_threads, double* out_k, double* out_g) {
  std::string err;
  if (!out_k || n_threads < 0) {
    feat_set_error(std::string(who) + ": null output or negative n_threads");
    return SK_ERR_INVALID;
  }
  const int rc = feat_check(who, xs, ys, kind, degree, params, true, err);
  if (rc) {
    feat_set_error(err);
    return rc;
  }
  const int64_t nx = xs->n, ny = ys ? ys->n : xs->n;
  if (nx == 0 || ny == 0) return SK_OK;
  std::vector<double> D((size_t)(nx * ny)), dx, dy;
  dots_host(xs, ys, n_threads, D.data(), &dx, &dy);
  const bool sym = !ys;
  switch (kind) {
    case kFeatRbf:
      apply_host<kFeatRbf>(D.data(), nx, ny, dx.data(), dy.data(), sym, degree, params, n_threads, out_k, out_g);
      break;
    case kFeatPoly:
      apply_host<kFeatPoly>(D.data(), nx, ny, dx.data(), dy.data(), sym, degree, params, n_threads, out_k, out_g);
      break;
    default:
      apply_host<kFeatSigmoid>(D.data(), nx, ny, dx.data(), dy.data(), sym, degree, params, n_threads, out_k, out_g);
  }
  return SK_OK;
}
}  // namespace

void feat_set_error(const std::string& msg) { g_feat_err = msg; }

std::vector<int32_t> feat_columns(const sk_features* xs, const sk_features* ys) {
  if (!ys || ys == xs) return xs->cols;
  std::vector<int32_t> u(xs->cols.size() + ys->cols.size());
  u.resize((size_t)(std::set_union(xs->cols.begin(), xs->cols.end(), ys->cols.begin(), ys->cols.end(), u.begin()) -
                    u.begin()));
  return u;
}

void feat_dense(const sk_features* fs, const std::vector<int32_t>& cols, double* out) {
  const int64_t d = (int64_t)cols.size();
  std::fill(out, out + (int64_t)fs->n * d, 0.0);
  for (int32_t i = 0; i < fs->n; ++i) {
    size_t c = 0;  // the row's indices ascend: one merge pass over the columns
    for (int64_t k = fs->row_ptr[i]; k < fs->row_ptr[i + 1]; ++k) {
      c = (size_t)(std::lower_bound(cols.begin() + c, cols.end(), fs->index[k]) - cols.begin());
      out[(int64_t)i * d + (int64_t)c] = fs->value[k];
    }
  }
}

int feat_check(const char* who, const sk_features* xs, const sk_features* ys, int kind, int degree,
               const double* params, bool need_params, std::string& err) {
  const std::string w = std::string(who) + ": ";
  if (!xs) {
    err = w + "null feature set";
    return SK_ERR_INVALID;
  }
  if (need_params) {
    if (kind < kFeatRbf || kind > kFeatSigmoid || !params) {
      err = w + "kind must be SK_FEAT_RBF, SK_FEAT_POLY or SK_FEAT_SIGMOID, with its parameters";
      return SK_ERR_INVALID;
    }
    if (kind == kFeatPoly && degree < 0) {
      err = w + "degree must be >= 0";
      return SK_ERR_INVALID;
    }
  }
  if (xs->n > kFeatMaxN || (ys && ys->n > kFeatMaxN)) {
    err = w + std::to_string(std::max(xs->n, ys ? ys->n : 0)) + " examples are over the limit of " +
          std::to_string(kFeatMaxN) + " (sk_feature_gram_shape: max_n)";
    return SK_ERR_UNSUPPORTED;
  }
  // (the union's size is at most the sum of the two sets' columns: checked
  // exactly, but only when the cheap bound is over)
  const int64_t rows = (int64_t)xs->n + (ys ? ys->n : 0);
  int64_t d = (int64_t)xs->cols.size() + (ys ? (int64_t)ys->cols.size() : 0);
  if (rows * d > kFeatMaxDense && ys) d = (int64_t)feat_columns(xs, ys).size();
  if (rows * d > kFeatMaxDense) {
    err = w + std::to_string(rows) + " examples x " + std::to_string(d) + " used columns are over the dense budget of " +
          std::to_string(kFeatMaxDense) + " entries (sk_feature_gram_shape: max_dense)";
    return SK_ERR_UNSUPPORTED;
  }
  return SK_OK;
}

}  // namespace sk

extern "C" {

const char* sk_features_last_error(void) { return sk::g_feat_err.c_str(); }

int sk_features_create(int32_t n, const int64_t* row_ptr, const int32_t* index, const double* value,
                       const int32_t* labels, sk_features** out) {
  if (!out) return SK_ERR_INVALID;
  *out = nullptr;
  if (n < 0 || !row_ptr || (row_ptr[n] > 0 && (!index || !value)) || row_ptr[0] != 0 || row_ptr[n] < 0) {
    sk::feat_set_error("sk_features_create: n >= 0, row_ptr[0] = 0 and the arrays are required");
    return SK_ERR_INVALID;
  }
  try {
    std::unique_ptr<sk_features> fs(new sk_features());
    fs->n = n;
    fs->row_ptr.assign(row_ptr, row_ptr + n + 1);
    fs->index.assign(index, index + row_ptr[n]);
    fs->value.assign(value, value + row_ptr[n]);
    if (labels)
      fs->labels.assign(labels, labels + n);
    else
      fs->labels.assign((size_t)n, 0);
    std::string err;
    const int rc = sk::finish(fs.get(), err, "sk_features_create");
    if (rc) {
      sk::feat_set_error(err);
      return rc;
    }
    *out = fs.release();
    return SK_OK;
  } catch (const std::bad_alloc&) {
    sk::feat_set_error("sk_features_create: host memory");
    return SK_ERR_ALLOC;
  }
}

int sk_features_parse(const char* text, size_t len, sk_features** out) {
  if (!out) return SK_ERR_INVALID;
  *out = nullptr;
  if (!text && len) return SK_ERR_INVALID;
  try {
    std::unique_ptr<sk_features> fs(new sk_features());
    std::string err;
    const int rc = sk::parse_text(text, len, fs.get(), err);
    if (rc) {
      sk::feat_set_error(err);
      return rc;
    }
    *out = fs.release();
    return SK_OK;
  } catch (const std::bad_alloc&) {
    sk::feat_set_error("sk_features_parse: host memory");
    return SK_ERR_ALLOC;
  }
}

int sk_features_read(const char* path, sk_features** out) {
  if (!out) return SK_ERR_INVALID;
  *out = nullptr;
  if (!path) return SK_ERR_INVALID;
  std::FILE* f = std::fopen(path, "rb");
  if (!f) {
    sk::feat_set_error(std::string("sk_features_read: cannot open ") + path);
    return SK_ERR_INVALID;
  }
  std::string text;
  try {
    char buf[1 << 16];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
  } catch (const std::bad_alloc&) {
    std::fclose(f);
    sk::feat_set_error("sk_features_read: host memory");
    return SK_ERR_ALLOC;
  }
  std::fclose(f);
  return sk_features_parse(text.data(), text.size(), out);
}

int sk_features_free(sk_features* fs) {
  if (!fs) return SK_OK;
  sk::feat_dots_forget(nullptr, fs);
  delete fs;
  return SK_OK;
}

int sk_features_shape(const sk_features* fs, int32_t* n, int32_t* d, int64_t* nnz) {
  if (!fs) return SK_ERR_INVALID;
  if (n) *n = fs->n;
  if (d) *d = (int32_t)fs->cols.size();
  if (nnz) *nnz = (int64_t)fs->index.size();
  return SK_OK;
}

int sk_features_labels(const sk_features* fs, int32_t* out) {
  if (!fs || (!out && fs->n)) return SK_ERR_INVALID;
  std::copy(fs->labels.begin(), fs->labels.end(), out);
  return SK_OK;
}

int sk_features_rows(const sk_features* fs, int64_t* row_ptr, int32_t* index, double* value) {
  if (!fs) return SK_ERR_INVALID;
  if (row_ptr) std::copy(fs->row_ptr.begin(), fs->row_ptr.end(), row_ptr);
  if (index) std::copy(fs->index.begin(), fs->index.end(), index);
  if (value) std::copy(fs->value.begin(), fs->value.end(), value);
  return SK_OK;
}

int sk_feature_gram_shape(int32_t* tile, int32_t* k_slice, int32_t* max_n, int64_t* max_dense) {
  if (tile) *tile = sk::kFeatTile;
  if (k_slice) *k_slice = sk::kFeatSlice;
  if (max_n) *max_n = sk::kFeatMaxN;
  if (max_dense) *max_dense = sk::kFeatMaxDense;
  return SK_OK;
}

int sk_feature_dots_host(const sk_features* xs, const sk_features* ys, int32_t n_threads, double* out) {
  try {
    std::string err;
    if (!out || n_threads < 0) return SK_ERR_INVALID;
    const int rc = sk::feat_check("sk_feature_dots_host", xs, ys, 0, 0, nullptr, false, err);
    if (rc) {
      sk::feat_set_error(err);
      return rc;
    }
    if (xs->n && (!ys || ys->n)) sk::dots_host(xs, ys, n_threads, out, nullptr, nullptr);
    return SK_OK;
  } catch (const std::bad_alloc&) {
    sk::feat_set_error("sk_feature_dots_host: host memory");
    return SK_ERR_ALLOC;
  }
}

int sk_feature_gram_host(const sk_features* xs, int32_t kind, int32_t degree, const double* params, int32_t n_threads,
                         double* out_k, double* out_g) {
  try {
    return sk::gram_host("sk_feature_gram_host", xs, nullptr, kind, degree, params, n_threads, out_k, out_g);
  } catch (const std::bad_alloc&) {
    sk::feat_set_error("sk_feature_gram_host: host memory");
    return SK_ERR_ALLOC;
  }
}

int sk_feature_gram_cross_host(const sk_features* test, const sk_features* train, int32_t kind, int32_t degree,
                               const double* params, int32_t n_threads, double* out_k) {
  try {
    if (!train) return SK_ERR_INVALID;
    return sk::gram_host("sk_feature_gram_cross_host", test, train, kind, degree, params, n_threads, out_k, nullptr);
  } catch (const std::bad_alloc&) {
    sk::feat_set_error("sk_feature_gram_cross_host: host memory");
    return SK_ERR_ALLOC;
  }
}

}  // extern "C"
