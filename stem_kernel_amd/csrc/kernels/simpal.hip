// Simple palindrome kernel on CDNA4 (gfx950): the reference's simpal tool.
//
// Reference: KernelFunc::operator()  simpal/simpal.cpp:236-266
//   K(x, y) = sum_a sum_b [mismatches(key_a, key_b) <= tolerance]
//             * exp(-|d_a - d_b|) * w_a * w_b
//   over the entries (key, d) -> w of the two examples' maps (Pals, :37-218),
//   double arithmetic, a term being (exp(-dist) * w_a) * w_b.
//
// Work item: up to kSimpalWaves pairs that share their y example (the host
// groups the pairs by column and orders the items by cost, largest first;
// workgroups draw them from a counter).  The y entries stream through LDS in
// tiles of kSimpalYTile, loaded once for all waves of the workgroup; wave w
// computes pair w of the item.  A lane holds kSimpalXBlock x entries in
// registers (x entry 64 r + lane of the current block of 64 * kSimpalXBlock),
// so one broadcast LDS read of a y entry (every lane the same address: no
// bank conflict) serves kSimpalXBlock terms per lane.  The last block of an
// example uses only the slots its entries reach (ceil(rest / 64)).
//
// Keys are 2 bits per letter in one 64-bit word (seed_length <= 32): the
// mismatch count is popcount(((a ^ b) | (a ^ b) >> 1) & 0x5555...).
//
// exp(-|d|) comes from a host-built table of libm's exp(-d), d = 0..745, in
// LDS, with one more slot holding 0: libm's exp(-d) is 0 from d = 746 on, and
// the index is min(|d|, 746), so no distance gives anything but the table's
// finite values.  A lane's gather of the table is the one LDS read per term
// that can meet bank conflicts.
//
// The bits of K(x, y) depend on x, y and the parameters alone: a pair is
// summed by one wave, each lane adding its terms in the fixed order (y tile,
// x block, y entry) into one accumulator per register slot, the slots then
// the lanes combined in a fixed tree.  No floating-point atomics.  Every term
// is >= 0, so the order costs no accuracy.
//
// LDS per workgroup: 748 * 8 + 1024 * 20 B = 26.5 KB, so two (and more)
// workgroups of 4 waves fit a CU's 160 KB.
#include <hip/hip_runtime.h>

#include "launch.h"

namespace sk {

namespace {

// One y tile against the first NR register slots of a block of x entries:
// per y entry a broadcast LDS read, then NR terms per lane.
template <int NR>
__device__ __forceinline__ void simpal_terms(const uint64_t* yk, const int32_t* yd, const double* yw,
                                             const double* et, int tn, int tol,
                                             const uint64_t (&ka)[kSimpalXBlock], const int32_t (&da)[kSimpalXBlock],
                                             const double (&wa)[kSimpalXBlock], double (&acc)[kSimpalXBlock]) {
#pragma unroll 2
  for (int j = 0; j < tn; ++j) {
    const uint64_t kb = yk[j];
    const int32_t db = yd[j];
    const double wb = yw[j];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      uint64_t v = ka[r] ^ kb;
      v = (v | (v >> 1)) & 0x5555555555555555ull;
      const int mm = __popcll(v);
      // dists are >= 0: the difference cannot overflow
      const int dd = da[r] - db;
      const unsigned ad = (unsigned)(dd < 0 ? -dd : dd);
      const double e = et[min(ad, (unsigned)kSimpalExpN)];
      const double term = (e * wa[r]) * wb;
      acc[r] += mm <= tol ? term : 0.0;
    }
  }
}

}  // namespace

__global__ void __launch_bounds__(64 * kSimpalWaves) sk_simpal_kernel(SimpalLaunch P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ unsigned long long s_item;
  constexpr int T = kSimpalYTile, XB = kSimpalXBlock, B = 64 * XB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // LDS: exp table [kSimpalExpN + 2] | y keys [T] | y weights [T] | y dists [T]
  double* et = reinterpret_cast<double*>(smem);
  uint64_t* yk = reinterpret_cast<uint64_t*>(et + kSimpalExpN + 2);
  double* yw = reinterpret_cast<double*>(yk + T);
  int32_t* yd = reinterpret_cast<int32_t*>(yw + T);

  for (int k = threadIdx.x; k <= kSimpalExpN; k += blockDim.x) et[k] = P.exp_tab[k];
  const int tol = P.tol;

  for (;;) {
    __syncthreads();  // the last item's tile and s_item are read
    if (threadIdx.x == 0) s_item = atomicAdd(P.item_counter, 1ull);
    __syncthreads();
    const unsigned long long item = s_item;
    if (item >= (unsigned long long)P.n_items) break;
    const int p0 = P.item_first[item], cnt = P.item_first[item + 1] - p0;
    const int y = P.ys[p0];
    const int y0 = P.yset.ex_off[y], ny = P.yset.ex_off[y + 1] - y0;
    const bool has = wave < cnt;  // this wave's pair of the item
    const int pr = p0 + (has ? wave : 0);
    const int x = P.xs[pr];
    const int x0 = P.xset.ex_off[x], nx = has ? P.xset.ex_off[x + 1] - x0 : 0;

    double acc[XB];
#pragma unroll
    for (int r = 0; r < XB; ++r) acc[r] = 0.0;

    for (int t0 = 0; t0 < ny; t0 += T) {
      const int tn = min(T, ny - t0);
      if (t0) __syncthreads();  // every wave is through the tile before
      for (int j = threadIdx.x; j < tn; j += blockDim.x) {
        yk[j] = P.yset.key[y0 + t0 + j];
        yw[j] = (double)P.yset.w[y0 + t0 + j];
        yd[j] = P.yset.dist[y0 + t0 + j];
      }
      __syncthreads();
      for (int xb = 0; xb < nx; xb += B) {
        // x entries of this block: slot r holds entry xb + 64 r + lane; past
        // the end a zero weight (the term is then exp * 0 * w_b = 0)
        uint64_t ka[XB];
        int32_t da[XB];
        double wa[XB];
#pragma unroll
        for (int r = 0; r < XB; ++r) {
          const int e = xb + 64 * r + lane;
          const bool ok = e < nx;
          ka[r] = ok ? P.xset.key[x0 + e] : 0ull;
          da[r] = ok ? P.xset.dist[x0 + e] : 0;
          wa[r] = ok ? (double)P.xset.w[x0 + e] : 0.0;
        }
        // register slots in use: the last block of an example may fill
        // fewer than XB (wave-uniform; a function of |P_x| alone)
        static_assert(XB == 4, "the cases below list the slot counts of XB = 4");
        switch (min(XB, (nx - xb + 63) >> 6)) {
          case 1: simpal_terms<1>(yk, yd, yw, et, tn, tol, ka, da, wa, acc); break;
          case 2: simpal_terms<2>(yk, yd, yw, et, tn, tol, ka, da, wa, acc); break;
          case 3: simpal_terms<3>(yk, yd, yw, et, tn, tol, ka, da, wa, acc); break;
          default: simpal_terms<XB>(yk, yd, yw, et, tn, tol, ka, da, wa, acc); break;
        }
      }
    }
    // the pair's value: slots in order, then the lanes' fixed tree
    double s = acc[0];
#pragma unroll
    for (int r = 1; r < XB; ++r) s += acc[r];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (has && lane == 0) P.out[P.oidx ? P.oidx[pr] : (int64_t)pr] = s;
  }
}

hipError_t launch_simpal(const SimpalLaunch& P, int grid, hipStream_t st) {
  SimpalLaunch a = P;
  void* args[] = {&a};
  return hipLaunchKernel(reinterpret_cast<const void*>(sk_simpal_kernel), dim3(grid), dim3(64 * kSimpalWaves), args,
                         simpal_lds_bytes(), st);
}

}  // namespace sk
