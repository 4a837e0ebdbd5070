// Examples as bytes (the SKEX format): exporting a range of a dataset,
// importing a buffer after checking every invariant the packer and the kernels
// rely on, and copying one example between datasets.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <iterator>
#include <new>
#include <string>
#include <vector>

#include "host/runtime_types.h"

namespace sk {
// ---- examples as bytes (a dataset built in rank shares, gathered) --------
// Layout: "SKEX", version 1, count; per example its label and every Example
// field in declaration order (PODs raw, vectors as u64 count + elements,
// strings as u32 length + bytes), little-endian as the host.
namespace {
struct ExWriter {
  uint8_t* buf;
  size_t cap, n = 0;
  void raw(const void* p, size_t b) {
    if (buf && n + b <= cap) std::memcpy(buf + n, p, b);
    n += b;
  }
  template <class T>
  void pod(const T& v) { raw(&v, sizeof(T)); }
  void str(const std::string& s) {
    pod((uint32_t)s.size());
    raw(s.data(), s.size());
  }
  template <class T>
  void vec(const std::vector<T>& v) {
    pod((uint64_t)v.size());
    raw(v.data(), v.size() * sizeof(T));
  }
};
struct ExReader {
  const uint8_t* buf;
  size_t size, n = 0;
  bool ok = true;
  void raw(void* p, size_t b) {
    if (!ok || b > size - n) {
      ok = false;
      return;
    }
    std::memcpy(p, buf + n, b);
    n += b;
  }
  template <class T>
  void pod(T& v) { raw(&v, sizeof(T)); }
  void str(std::string& s) {
    uint32_t l = 0;
    pod(l);
    if (!ok || l > size - n) {
      ok = false;
      return;
    }
    s.assign(reinterpret_cast<const char*>(buf + n), l);
    n += l;
  }
  template <class T>
  void vec(std::vector<T>& v) {
    uint64_t c = 0;
    pod(c);
    if (!ok || c > (size - n) / sizeof(T)) {
      ok = false;
      return;
    }
    v.resize((size_t)c);
    raw(v.data(), (size_t)c * sizeof(T));
  }
};
template <class IO, class E>
void example_fields(IO& io, E& X) {
  io.pod(X.len);
  io.pod(X.n_rows);
  uint8_t hb = X.has_bp ? 1 : 0;  // (a byte on the wire, not a bool's object representation)
  io.pod(hb);
  if constexpr (std::is_same_v<IO, ExReader>) X.has_bp = hb != 0;
  uint32_t nr = (uint32_t)X.rows.size();
  io.pod(nr);
  if constexpr (std::is_same_v<IO, ExReader>) {
    if (!io.ok || nr > io.size - io.n) {
      io.ok = false;
      return;
    }
    X.rows.resize(nr);
  }
  for (auto& r : X.rows) io.str(r);
  io.vec(X.prof5);
  io.pod(X.n_seqs);
  io.vec(X.pos_weight);
  io.vec(X.bpp);
  io.vec(X.first);
  io.vec(X.last);
  io.vec(X.weight);
  io.vec(X.edge_off);
  io.vec(X.edge_to);
  io.vec(X.edge_gaps);
  io.vec(X.bpf_off);
  io.vec(X.bpf_code);
  io.vec(X.bpf_p);
  io.vec(X.roots);
  io.vec(X.max_pa);
}
template <class IO, class E>
void protein_fields(IO& io, E& X) {
  uint8_t pb = X.protein ? 1 : 0;
  io.pod(pb);
  if constexpr (std::is_same_v<IO, ExReader>) X.protein = pb != 0;
  io.vec(X.aa_prof);
}
template <class IO, class E>
void palindrome_fields(IO& io, E& X) {
  uint8_t pb = X.pal ? 1 : 0;
  io.pod(pb);
  if constexpr (std::is_same_v<IO, ExReader>) X.pal = pb != 0;
  io.pod(X.pal_seed);
  io.vec(X.pal_key);
  io.vec(X.pal_dist);
  io.vec(X.pal_w);
}
constexpr uint32_t kExMagic = 0x58454b53u;  // "SKEX"

// What simpal.hip relies on in a palindrome example: entries in map order
// without duplicates, keys of seed_length letters, dists >= 0, finite
// weights >= 0.
bool palindromes_valid(const Example& X) {
  const size_t m = X.pal_key.size();
  if (X.pal_seed < 1 || X.pal_seed > 32 || X.pal_dist.size() != m || X.pal_w.size() != m) return false;
  if (m > (size_t)INT32_MAX) return false;
  for (size_t k = 0; k < m; ++k) {
    if (X.pal_seed < 32 && (X.pal_key[k] >> (2 * X.pal_seed)) != 0) return false;
    if (X.pal_dist[k] < 0 || !(X.pal_w[k] >= 0.0f) || !std::isfinite(X.pal_w[k])) return false;
    if (k && !(X.pal_key[k - 1] < X.pal_key[k] ||
               (X.pal_key[k - 1] == X.pal_key[k] && X.pal_dist[k - 1] < X.pal_dist[k])))
      return false;
  }
  return true;
}

// The invariants example_build.cpp establishes and the packer and kernels
// rely on (sizes, offsets, children numbered before parents, positions and
// bp-frequency codes in range): an imported example must hold them all.
bool example_valid(const Example& X) {
  const size_t L = X.len >= 0 ? (size_t)X.len : 0;
  if (X.len < 0 || X.n_rows < 1 || X.rows.size() != (size_t)X.n_rows) return false;
  for (const auto& r : X.rows)
    if (r.size() != L) return false;
  const bool no_rna = !X.has_bp && X.prof5.empty() && X.pos_weight.empty() && X.bpp.empty() && X.first.empty() &&
                      X.last.empty() && X.weight.empty() && X.edge_off.empty() && X.edge_to.empty() &&
                      X.edge_gaps.empty() && X.bpf_off.empty() && X.bpf_code.empty() && X.bpf_p.empty() &&
                      X.roots.empty() && X.max_pa.empty();
  if (X.pal)  // its entries, and none of the RNA or protein fields
    return !X.protein && X.aa_prof.empty() && X.n_rows == 1 && no_rna && palindromes_valid(X);
  if (X.pal_seed != 0 || !X.pal_key.empty() || !X.pal_dist.empty() || !X.pal_w.empty()) return false;
  if (X.protein) {
    // integer counts, every column summing to the row count (< 4,096 rows),
    // and none of the RNA fields
    if (X.n_rows >= kAaMaxRows || X.n_seqs != (float)X.n_rows || X.aa_prof.size() != L * sk::kAaSlots) return false;
    for (size_t i = 0; i < L; ++i) {
      float sum = 0.0f;
      for (int k = 0; k < sk::kAaSlots; ++k) {
        const float c = X.aa_prof[i * sk::kAaSlots + k];
        if (!(c >= 0.0f) || c != std::floor(c)) return false;
        sum += c;
      }
      if (sum != (float)X.n_rows) return false;
    }
    return !X.has_bp && X.prof5.empty() && X.pos_weight.empty() && X.bpp.empty() && X.first.empty() &&
           X.last.empty() && X.weight.empty() && X.edge_off.empty() && X.edge_to.empty() && X.edge_gaps.empty() &&
           X.bpf_off.empty() && X.bpf_code.empty() && X.bpf_p.empty() && X.roots.empty() && X.max_pa.empty();
  }
  if (!X.aa_prof.empty()) return false;
  if (X.prof5.size() != L * 5) return false;
  const size_t nn = X.first.size();
  if (X.last.size() != nn || X.weight.size() != nn) return false;
  if (X.edge_off.size() != nn + 1 || X.bpf_off.size() != nn + 1 || X.edge_off[0] != 0 || X.bpf_off[0] != 0)
    return false;
  for (size_t v = 0; v < nn; ++v) {
    if (X.edge_off[v + 1] < X.edge_off[v] || X.bpf_off[v + 1] < X.bpf_off[v]) return false;
    if (X.first[v] > X.last[v] || X.last[v] >= L) return false;
  }
  if (X.edge_to.size() != X.edge_off[nn] || X.edge_gaps.size() != X.edge_off[nn]) return false;
  if (X.bpf_code.size() != X.bpf_off[nn] || X.bpf_p.size() != X.bpf_off[nn]) return false;
  for (size_t v = 0; v < nn; ++v)
    for (uint32_t k = X.edge_off[v]; k < X.edge_off[v + 1]; ++k)
      if (X.edge_to[k] >= v) return false;  // children before parents
  for (uint8_t c : X.bpf_code)
    if (c >= 16) return false;
  for (uint32_t r : X.roots)
    if (r >= nn) return false;
  if (X.has_bp) {
    if (X.bpp.size() != (L > 1 ? L * (L - 1) / 2 : 0) || X.pos_weight.size() != L || X.max_pa.size() != nn)
      return false;
  } else if (nn != 0) {
    return false;
  }
  return true;
}
}  // namespace

}  // namespace sk

extern "C" {

int sk_dataset_add_copy(sk_dataset* dst, const sk_dataset* src, int32_t i) {
  if (!dst || !src || i < 0 || (size_t)i >= src->ex.size()) return SK_ERR_INVALID;
  if (dst->uploaded || sk::ds_mixes(dst, sk::ex_sort(src->ex[(size_t)i])) ||
      (src->ex[(size_t)i].pal && sk::pal_seed_differs(dst, src->ex[(size_t)i].pal_seed)))
    return SK_ERR_INVALID;
  try {
    dst->ex.push_back(src->ex[(size_t)i]);
    dst->labels.push_back(src->labels[(size_t)i]);
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
  return SK_OK;
}

int sk_dataset_export(const sk_dataset* ds, int32_t first, int32_t count, uint8_t* buf, size_t cap,
                      size_t* size) {
  if (!ds || !size || first < 0 || count < 0 || (size_t)first + (size_t)count > ds->ex.size())
    return SK_ERR_INVALID;
  sk::ExWriter w{buf, buf ? cap : 0};
  // version 2 = version 1 plus, per example, the protein fields; written only
  // when the range holds a protein example (RNA exports stay version 1)
  // version 3 = version 2 plus, per example, the palindrome fields; written
  // only when the range holds a palindrome example
  bool prot = false, pal = false;
  for (int32_t i = first; i < first + count; ++i) {
    prot = prot || ds->ex[(size_t)i].protein;
    pal = pal || ds->ex[(size_t)i].pal;
  }
  prot = prot || pal;
  w.pod(sk::kExMagic);
  w.pod((uint32_t)(pal ? 3 : prot ? 2 : 1));
  w.pod((uint32_t)count);
  for (int32_t i = first; i < first + count; ++i) {
    w.str(ds->labels[(size_t)i]);
    sk::example_fields(w, const_cast<sk::Example&>(ds->ex[(size_t)i]));
    if (prot) sk::protein_fields(w, const_cast<sk::Example&>(ds->ex[(size_t)i]));
    if (pal) sk::palindrome_fields(w, const_cast<sk::Example&>(ds->ex[(size_t)i]));
  }
  *size = w.n;
  return buf && w.n > cap ? SK_ERR_RANGE : SK_OK;
}

int sk_dataset_import(sk_dataset* ds, const uint8_t* buf, size_t size) {
  if (!ds || (!buf && size)) return SK_ERR_INVALID;
  if (ds->uploaded) return SK_ERR_INVALID;
  sk::ExReader r{buf, size};
  uint32_t magic = 0, ver = 0, count = 0;
  r.pod(magic);
  r.pod(ver);
  r.pod(count);
  if (!r.ok || magic != sk::kExMagic || ver < 1 || ver > 3) return SK_ERR_INVALID;
  std::vector<sk::Example> ex;
  std::vector<std::string> lab;
  try {
    for (uint32_t i = 0; i < count && r.ok; ++i) {
      lab.emplace_back();
      r.str(lab.back());
      ex.emplace_back();
      sk::example_fields(r, ex.back());
      if (ver >= 2) sk::protein_fields(r, ex.back());
      if (ver == 3) sk::palindrome_fields(r, ex.back());
    }
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
  if (!r.ok || r.n != size) return SK_ERR_INVALID;  // nothing appended from a malformed buffer
  for (const sk::Example& X : ex)
    if (!sk::example_valid(X)) return SK_ERR_INVALID;
  // a dataset is of one sort (and, palindromes, one seed_length): the
  // buffer's examples are of one sort, the dataset's
  for (const sk::Example& X : ex)
    if (sk::ex_sort(X) != sk::ex_sort(ex[0]) || sk::ds_mixes(ds, sk::ex_sort(X)) ||
        (X.pal && (X.pal_seed != ex[0].pal_seed || sk::pal_seed_differs(ds, X.pal_seed))))
      return SK_ERR_INVALID;
  try {
    ds->ex.insert(ds->ex.end(), std::make_move_iterator(ex.begin()), std::make_move_iterator(ex.end()));
    ds->labels.insert(ds->labels.end(), lab.begin(), lab.end());
  } catch (const std::bad_alloc&) {
    return SK_ERR_ALLOC;
  }
  return SK_OK;
}

}  // extern "C"
