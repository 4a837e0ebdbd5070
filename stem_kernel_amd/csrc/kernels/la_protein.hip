// Protein local-alignment kernel on CDNA4 (gfx950): the reference's la_kernel.
//
// Reference: BPLAKernel<double,AAMData>::operator()  bpla_kernel/bpla_kernel.cpp:159-174
//   (instantiated at bpla_kernel.cpp:406, built by la_main.cpp:131-135, noBP)
//   local_alignment_exp :64-115, local_alignment_max :117-157, LAScore :16-45
//   over AAProfileSequence columns of 24 integer counts (common/aaprofile.cpp:49-60).
//
// Both kernels run bpla.hip's systolic schedule (sk_bpla_kernel): one
// wavefront per pair, lane l owns DP rows i = 64*strip + l + 1 and computes
// column j of its row at step t, one step behind lane l-1, so the cell above
// is lane l-1's previous output (DPP wave_shr) and the diagonal one what the
// lane received a step earlier; strips are streamed, the strip boundary row
// goes through a per-wave LDS row.  FP64 throughout.
//
// exp mode uses the identity of the reference's recurrences that bpla.hip's
// fast path uses: X2 and Y2 only sum M (bpla_kernel.cpp:108-109), so
// 1 + X2[n][m] + Y2[n][m] + M[n][m] = 1 + the sum of M over all cells.  Each
// lane sums its cells; the terms are positive, a sum past the double range is
// inf as in the reference, and a pair's sum never meets another pair's.
//
// Code kernel (sk_la_prot_code_kernel): both examples have one residue kind
// per column (single sequences, identical rows), so LAScore is table[a][b] and
// the match factor one of 24x24 constants: an LDS table of exp(beta * t[a][b])
// (SW: t[a][b]), row = y residue, column = x residue, 1 (SW: 0) where either
// is "other" (an empty column scores 0, bpla_kernel.cpp:41).  No exp per cell.
// LDS: the table (4,608 B), then per wave 3 boundary rows and the y codes,
// 25 B per y column: with one wave a y of up to 6,366 residues fits 160 KiB.
//
// Profile kernel (sk_la_prot_prof_kernel): alignments.  Per row the lane holds
// u_l = sum_k t[k][l] x_k (23 doubles); a cell's score is
// (sum_l u_l y_l) / n with the float weight n = (sum_k x_k)(sum_l y_l): counts
// are integers and the host admits fewer than 4,096 rows, so every float
// product and partial sum of the reference's n is exact and equals this one.
// exp is the device library's.  LDS: per wave 3 boundary rows and the y
// columns as 24 floats (slot 23 holds the column's sum over the letters),
// 120 B per y column: with one wave a y of up to 1,326 columns.
// Workgroups have 4 waves, halved by the host while the LDS does not fit
// (run_la_protein); past the limits above it returns SK_ERR_UNSUPPORTED.
#include <hip/hip_runtime.h>

#include "bpla_fast.h"
#include "launch.h"

namespace sk {

namespace {

constexpr int kNA = kAaSlots - 1;  // 23 letters

__device__ __forceinline__ unsigned long long next_pair(unsigned long long* counter, int lane) {
  unsigned long long pr = 0;
  if (lane == 0) pr = atomicAdd(counter, 1ull);
  return ((unsigned long long)__builtin_amdgcn_readlane((unsigned)(pr >> 32), 0) << 32) |
         (unsigned)__builtin_amdgcn_readlane((unsigned)pr, 0);
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One cell from its match term and its three neighbours (up: (i-1, j),
// d: (i-1, j-1), a: (i, j-1)).  exp: e = the factor exp(beta * score); SW: e =
// the score.
template <bool SW>
__device__ __forceinline__ void la_cell(double e, double dM, double dX, double dY, double upM,
                                        double upX, double aM, double aX, double aY, double bg,
                                        double be, double gap, double ext, double& nM, double& nX,
                                        double& nY) {
  if (!SW) {
    nM = e * (1.0 + dX + dY + dM);
    nX = bg * upM + be * upX;
    nY = bg * (aM + aX) + be * aY;
  } else {
    double v = fmax(0.0, dM);
    v = fmax(v, dX);
    v = fmax(v, dY);
    nM = v + e;
    nX = fmax(upM + gap, upX + ext);
    nY = fmax(fmax(aM + gap, aX + gap), aY + ext);
  }
}

// the pair's value from the lanes' sums (exp) or maxima (SW)
template <bool SW>
__device__ __forceinline__ double la_reduce(double acc) {
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(acc, off, 64);
    acc = SW ? fmax(acc, o) : acc + o;
  }
  return SW ? acc : 1.0 + acc;
}

}  // namespace

template <bool SW>
__global__ void __launch_bounds__(256) sk_la_prot_code_kernel(LaProtLaunch P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int maxlen = P.lds_max_len;  // even
  // LDS: factor table [24 y][24 x] | per wave: bM, bX, bY [maxlen+2] | y codes [maxlen]
  double* ft = reinterpret_cast<double*>(smem);
  unsigned char* wbase = smem + kAaSlots * kAaSlots * 8 + (size_t)wave * la_prot_code_wave_lds_bytes(maxlen);
  double* bM = reinterpret_cast<double*>(wbase);
  double* bX = bM + (maxlen + 2);
  double* bY = bX + (maxlen + 2);
  uint8_t* ycode = reinterpret_cast<uint8_t*>(bY + (maxlen + 2));

  for (int k = threadIdx.x; k < kAaSlots * kAaSlots; k += blockDim.x) {
    const int b = k / kAaSlots, a = k - b * kAaSlots;  // y residue, x residue
    double v = SW ? 0.0 : 1.0;
    if (a < kNA && b < kNA) v = SW ? P.table[a * kNA + b] : exp(P.beta * P.table[a * kNA + b]);
    ft[k] = v;
  }
  __syncthreads();
  const double gap = P.gap, ext = P.ext, bg = P.beta_gap, be = P.beta_ext;

  for (;;) {
    const unsigned long long pr = next_pair(P.pair_counter, lane);
    if ((int64_t)pr >= P.n_pairs) break;
    const int x = P.xs[pr], y = P.ys[pr];
    const int Lx = P.xset.ex_len[x], Ly = P.yset.ex_len[y];
    const uint8_t* xcode = P.xset.code + P.xset.ex_pos_base[x];
    const uint8_t* yg = P.yset.code + P.yset.ex_pos_base[y];
    for (int j = lane; j < Ly; j += 64) ycode[j] = yg[j];
    // a strip takes Lys = max(Ly, 64) steps (bpla.hip: lane 0 reads boundary
    // column j at least a step after lane 63 wrote it, and before lane 63
    // overwrites it with the next strip's row)
    const int Lys = max(Ly, 64);
    for (int j = lane; j <= Lys; j += 64) {  // row 0 (bpla_kernel.cpp:89-95)
      bM[j] = 0.0;
      bX[j] = 0.0;
      bY[j] = 0.0;
    }
    wave_sync();

    double acc = 0.0;  // exp: sum of M over the lane's cells; SW: their maximum
    if (Lx > 0 && Ly > 0) {
      const int nstrips = (Lx + 63) / 64;
      int strip = 0, j = 1 - lane;
      int i = lane + 1;
      bool row_ok = i <= Lx;
      // the x residue of the current row (the table column) and the next row's
      int xa = row_ok ? xcode[i - 1] : kNA;
      int nxa = i + 64 <= Lx ? xcode[i + 63] : kNA;
      double lM = 0.0, lX = 0.0, lY = 0.0;  // my outputs of the previous step (i, j-1)
      double dM = 0.0, dX = 0.0, dY = 0.0;  // what I received last step: (i-1, j-1)
      const int T = (nstrips - 1) * Lys + ((Lx - 1) & 63) + Ly;
      for (int t = 0; t < T; ++t) {
        // lane 0 takes row i-1 from the boundary row (a wave-uniform column)
        const int jb = __builtin_amdgcn_readfirstlane(j);
        const int jr = jb >= 1 && jb <= Ly ? jb : 0;
        const double b0M = bM[jr], b0X = bX[jr], b0Y = bY[jr];
        const double upM = wave_shr1(lM, strip == 0 ? 0.0 : b0M);
        const double upX = wave_shr1(lX, strip == 0 ? 0.0 : b0X);
        const double upY = wave_shr1(lY, strip == 0 ? 0.0 : b0Y);
        if (j >= 1 && j <= Ly) {
          const double e = ft[(int)ycode[j - 1] * kAaSlots + xa];
          const bool c1 = j == 1;  // column 0 is zero
          const double aM = c1 ? 0.0 : lM, aX = c1 ? 0.0 : lX, aY = c1 ? 0.0 : lY;
          double nM, nX, nY;
          la_cell<SW>(e, dM, dX, dY, upM, upX, aM, aX, aY, bg, be, gap, ext, nM, nX, nY);
          if (row_ok) {
            lM = nM;
            lX = nX;
            lY = nY;
            acc = SW ? fmax(acc, nM) : acc + nM;
          }
          if (lane == 63) {
            bM[j] = nM;
            bX[j] = nX;
            bY[j] = nY;
          }
        }
        dM = upM;
        dX = upX;
        dY = upY;
        if (++j > Lys) {  // next strip: row i + 64, column 1
          j = 1;
          ++strip;
          i += 64;
          row_ok = i <= Lx;
          xa = nxa;
          nxa = i + 64 <= Lx ? xcode[i + 63] : kNA;
          dM = dX = dY = 0.0;
        }
      }
    }
    wave_sync();
    const double r = la_reduce<SW>(acc);
    if (lane == 0) P.out[P.oidx ? P.oidx[pr] : (int64_t)pr] = r;
    wave_sync();
  }
}

template <bool SW>
__global__ void __launch_bounds__(256) sk_la_prot_prof_kernel(LaProtLaunch P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int maxlen = P.lds_max_len;  // even
  // LDS: table [24][24] ([x][y], zero padded) | per wave: bM, bX, bY [maxlen+2] |
  // y columns [maxlen][24] float
  double* tb = reinterpret_cast<double*>(smem);
  unsigned char* wbase = smem + kAaSlots * kAaSlots * 8 + (size_t)wave * la_prot_prof_wave_lds_bytes(maxlen);
  double* bM = reinterpret_cast<double*>(wbase);
  double* bX = bM + (maxlen + 2);
  double* bY = bX + (maxlen + 2);
  float* ycol = reinterpret_cast<float*>(bY + (maxlen + 2));

  for (int k = threadIdx.x; k < kAaSlots * kAaSlots; k += blockDim.x) {
    const int a = k / kAaSlots, b = k - a * kAaSlots;
    tb[k] = a < kNA && b < kNA ? P.table[a * kNA + b] : 0.0;
  }
  __syncthreads();
  const double beta = P.beta, gap = P.gap, ext = P.ext, bg = P.beta_gap, be = P.beta_ext;

  for (;;) {
    const unsigned long long pr = next_pair(P.pair_counter, lane);
    if ((int64_t)pr >= P.n_pairs) break;
    const int x = P.xs[pr], y = P.ys[pr];
    const int Lx = P.xset.ex_len[x], Ly = P.yset.ex_len[y];
    const float* xprof = P.xset.prof + (size_t)P.xset.ex_pos_base[x] * kAaSlots;
    const float* yprof = P.yset.prof + (size_t)P.yset.ex_pos_base[y] * kAaSlots;
    for (int k = lane; k < Ly * kAaSlots; k += 64) ycol[k] = yprof[k];
    wave_sync();
    for (int j = lane; j < Ly; j += 64) {  // slot 23 := the column's sum over the letters
      float s = 0.0f;
      for (int l = 0; l < kNA; ++l) s += ycol[j * kAaSlots + l];
      ycol[j * kAaSlots + kNA] = s;
    }
    const int Lys = max(Ly, 64);
    for (int j = lane; j <= Lys; j += 64) {  // row 0 (bpla_kernel.cpp:89-95)
      bM[j] = 0.0;
      bX[j] = 0.0;
      bY[j] = 0.0;
    }
    wave_sync();

    double acc = 0.0;
    if (Lx > 0 && Ly > 0) {
      const int nstrips = (Lx + 63) / 64;
      int strip = 0, j = 1 - lane;
      int i = lane + 1;
      bool row_ok = i <= Lx;
      // LAScore's numerator factored per row: v = sum_l u_l y_l with
      // u_l = sum_k table[k][l] x_k; xs = sum_k x_k (exact in float)
      double u[kNA];
      float xs = 0.0f;
      auto load_row = [&](int row) {  // row: 1-based, <= Lx
#pragma unroll
        for (int l = 0; l < kNA; ++l) u[l] = 0.0;
        xs = 0.0f;
        const float* xr = xprof + (size_t)(row - 1) * kAaSlots;
        for (int k = 0; k < kNA; ++k) {
          const float c = xr[k];
          if (c != 0.0f) {
            xs += c;
            const double cd = (double)c;
#pragma unroll
            for (int l = 0; l < kNA; ++l) u[l] = __builtin_fma(tb[k * kAaSlots + l], cd, u[l]);
          }
        }
      };
#pragma unroll
      for (int l = 0; l < kNA; ++l) u[l] = 0.0;
      if (row_ok) load_row(i);
      double lM = 0.0, lX = 0.0, lY = 0.0;
      double dM = 0.0, dX = 0.0, dY = 0.0;
      const int T = (nstrips - 1) * Lys + ((Lx - 1) & 63) + Ly;
      for (int t = 0; t < T; ++t) {
        const int jb = __builtin_amdgcn_readfirstlane(j);
        const int jr = jb >= 1 && jb <= Ly ? jb : 0;
        const double b0M = bM[jr], b0X = bX[jr], b0Y = bY[jr];
        const double upM = wave_shr1(lM, strip == 0 ? 0.0 : b0M);
        const double upX = wave_shr1(lX, strip == 0 ? 0.0 : b0X);
        const double upY = wave_shr1(lY, strip == 0 ? 0.0 : b0Y);
        if (j >= 1 && j <= Ly) {
          const float* yc = ycol + (j - 1) * kAaSlots;
          double v = 0.0;
#pragma unroll
          for (int l = 0; l < kNA; ++l) v = __builtin_fma(u[l], (double)yc[l], v);
          const float n = xs * yc[kNA];
          const double s = n == 0.0f ? 0.0 : v / (double)n;
          const double e = SW ? s : exp(beta * s);
          const bool c1 = j == 1;
          const double aM = c1 ? 0.0 : lM, aX = c1 ? 0.0 : lX, aY = c1 ? 0.0 : lY;
          double nM, nX, nY;
          la_cell<SW>(e, dM, dX, dY, upM, upX, aM, aX, aY, bg, be, gap, ext, nM, nX, nY);
          if (row_ok) {
            lM = nM;
            lX = nX;
            lY = nY;
            acc = SW ? fmax(acc, nM) : acc + nM;
          }
          if (lane == 63) {
            bM[j] = nM;
            bX[j] = nX;
            bY[j] = nY;
          }
        }
        dM = upM;
        dX = upX;
        dY = upY;
        if (++j > Lys) {
          j = 1;
          ++strip;
          i += 64;
          row_ok = i <= Lx;
          if (row_ok) load_row(i);
          dM = dX = dY = 0.0;
        }
      }
    }
    wave_sync();
    const double r = la_reduce<SW>(acc);
    if (lane == 0) P.out[P.oidx ? P.oidx[pr] : (int64_t)pr] = r;
    wave_sync();
  }
}

static hipError_t la_launch(const void* fn, const LaProtLaunch& P, int grid, int nwaves, size_t lds,
                            hipStream_t st) {
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  LaProtLaunch a = P;
  void* args[] = {&a};
  return hipLaunchKernel(fn, dim3(grid), dim3(64 * nwaves), args, lds, st);
}

hipError_t launch_la_prot_code(const LaProtLaunch& P, int grid, int nwaves, hipStream_t st) {
  const size_t lds = la_prot_code_lds_bytes(P.lds_max_len, nwaves);
  const void* fn = P.sw ? reinterpret_cast<const void*>(sk_la_prot_code_kernel<true>)
                        : reinterpret_cast<const void*>(sk_la_prot_code_kernel<false>);
  return la_launch(fn, P, grid, nwaves, lds, st);
}

hipError_t launch_la_prot_prof(const LaProtLaunch& P, int grid, int nwaves, hipStream_t st) {
  const size_t lds = la_prot_prof_lds_bytes(P.lds_max_len, nwaves);
  const void* fn = P.sw ? reinterpret_cast<const void*>(sk_la_prot_prof_kernel<true>)
                        : reinterpret_cast<const void*>(sk_la_prot_prof_kernel<false>);
  return la_launch(fn, P, grid, nwaves, lds, st);
}

}  // namespace sk
