// Column model of the consensus (alifold-style) fold (fold_ali.hip; DESIGN.md
// §9): the pair-type table the single-sequence fold shares, the per-row type
// of two alignment columns and the covariance score that decides which
// column pairs may form.  Host and device run the same code: the host walks
// the --noLonelyPairs chains over "allowed", the kernel fills its per-cell
// tables from it.
#pragma once

#include <cstdint>

#if defined(__HIP__)
#define SK_ALI_HD __host__ __device__
#else
#define SK_ALI_HD
#endif

namespace sk {

// pair type of codes (a, b), a * 4 + b -> 4 bits of a 64-bit constant (no
// memory access: a __constant__ table indexed per thread is a vector load):
// {0,0,0,5, 0,0,1,0, 0,2,0,4, 6,0,3,0}  CG1 GC2 GU3 UG4 AU5 UA6
constexpr uint64_t kFoldPairBits = 0x306402001005000ull;

// the codes a * 4 + b of pair type t (1..6)
constexpr int ali_pair_letters(int t) {
  for (int k = 0; k < 16; ++k)
    if ((int)((kFoldPairBits >> (4 * k)) & 0xfu) == t) return k;
  return 0;
}
// Hamming distance of the letters of pair types k < l (1..6), 2 bits each in
// the order (1,2) (1,3) .. (1,6) (2,3) .. (5,6)
constexpr uint32_t ali_hamming_bits() {
  uint32_t bits = 0;
  int idx = 0;
  for (int k = 1; k <= 5; ++k)
    for (int l = k + 1; l <= 6; ++l, ++idx) {
      const int a = ali_pair_letters(k), b = ali_pair_letters(l);
      const uint32_t h = (uint32_t)((a >> 2) != (b >> 2)) + (uint32_t)((a & 3) != (b & 3));
      bits |= h << (2 * idx);
    }
  return bits;
}
constexpr uint32_t kAliHammingBits = ali_hamming_bits();

// rows of one alignment the 16-bit type counters hold
constexpr int kAliMaxRows = 32767;

// type of columns (i, j) in one row, codes a = c[i], b = c[j] (A C G U =
// 0..3, blank -1): 7 both blank, else the table's type (GU/UG -> 0 under
// --noGU), 0 = no pair
SK_ALI_HD inline int ali_row_type(int a, int b, bool ngu) {
  if (a < 0 && b < 0) return 7;
  if (a < 0 || b < 0) return 0;
  const int t = (int)((kFoldPairBits >> (4 * (a * 4 + b))) & 0xfu);
  return (ngu && (t == 3 || t == 4)) ? 0 : t;
}
// the type the loop energies read (0 as 7), and the reversed inner type of a stack
SK_ALI_HD inline int ali_energy_type(int t) { return t ? t : 7; }
SK_ALI_HD inline int ali_reversed(int e) { return e == 7 ? 7 : ((e - 1) ^ 1) + 1; }

// rows per type of one column pair, 16 bits each (no per-thread array)
struct AliCounts {
  uint64_t lo = 0, hi = 0;  // types 0..3, 4..7
  SK_ALI_HD void add(int t) {
    const uint64_t one = 1ull << (16 * (t & 3));
    if (t < 4) lo += one; else hi += one;
  }
  SK_ALI_HD int get(int t) const { return (int)(((t < 4 ? lo : hi) >> (16 * (t & 3))) & 0xffffu); }
};

// covariance score of a column pair of n_rows rows (dcal/mol) and whether
// the pair may form at span d = j - i
SK_ALI_HD inline bool ali_allowed(const AliCounts& pf, int n_rows, int d, int64_t* pscore) {
  int64_t score = 0;
  int idx = 0;
  for (int k = 1; k <= 5; ++k)
    for (int l = k + 1; l <= 6; ++l, ++idx)
      score += (int64_t)pf.get(k) * pf.get(l) * (int64_t)((kAliHammingBits >> (2 * idx)) & 3u);
  const int64_t ps = (100 * score) / n_rows - 100 * (int64_t)pf.get(0) - 25 * (int64_t)pf.get(7);
  *pscore = ps;
  return d >= 4 && 2 * pf.get(0) <= n_rows && ps >= -200;
}

}  // namespace sk
