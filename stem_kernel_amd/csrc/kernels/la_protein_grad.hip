// Gradients of the protein local-alignment kernel on CDNA4 (gfx950).
//
// Reference: BPLAKernel<double,AAMData>::compute_gradients
//   bpla_kernel/bpla_kernel.cpp:385-401 (instantiated at :406): BPLA_Forward
//   :178-243, BPLA_Backward :245-305, BPLA_ForwardBackword :325-383, LAScore
//   :16-45 over AAProfileSequence columns, with p_left = p_right = 0,
//   p_unpair = 1 on both examples (what the noBP kernel scores) and alpha = 1.
//   Outputs per pair: the forward value and d/d(alpha, beta, gap, ext); the
//   alpha slot is +0.0 (w_pair = 0).
//
// The value is compute_gradients' return value, NOT operator()'s (the value
// of la_protein.hip): the forward model starts alignments through F_LX = 1,
// F_LY = j, which weights alignment starts differently.  It is the model the
// reference's optimizer differentiates, and it is not symmetric in (x, y).
//
// Both kernels run sk_bpla_grad_wave_kernel's schedule (bpla_grad.hip:258-282,
// where the gathered backward recurrences and the closed forms of the L and R
// states are derived): one wavefront per pair, persistent waves pulling pairs
// from a counter;
//   1. the BACKWARD pass on the streamed-strip systolic schedule played in
//      reverse time (lane l owns rows 64s+l+1; row a+1 lives one lane up; the
//      strip boundary row goes through LDS), storing B_M, B_IX, B_IY per
//      (state, step, lane) in the wave's HBM table: 24 B per cell, 512
//      contiguous bytes per state per step;
//   2. the FORWARD pass recomputes F step by step, reads the stored B of the
//      same (step, lane) a step ahead, and adds the cell's terms into the
//      lane's beta, gap, ext and value sums; one butterfly at the end.
// The only atomic is the pair counter.  Sums run in another order than the
// reference's, but in one order per pair whatever the batch: a pair's bits do
// not depend on the pairs around it.
//
// Code kernel (sk_la_prot_grad_kernel<false>): both examples have one residue
// kind per column.  Two 24x24 LDS tables, exp(beta * t[a][b]) and t[a][b],
// row = y residue, column = x residue ("other": factor 1, score 0); no exp per
// cell; d/d beta's match term is t * v.  LDS: 9,216 B of tables, then per
// wave 3 boundary rows and the y codes, 25 B per y column.
//
// Profile kernel (sk_la_prot_grad_kernel<true>): alignments.  Per row the lane
// holds u_l = sum_k t[k][l] x_k; the cell's score is (sum_l u_l y_l) / n with
// the exact float n (la_protein.hip:29-36); one device exp per cell per pass.
// LDS: the table (4,608 B), then per wave 3 boundary rows and the y columns
// as 24 floats, 120 B per y column.
//
// The y limits follow from a one-wave workgroup filling the CU's 160 KiB
// (la_prot_grad_max_y, launch.h); the x length is not limited by the kernels.
#include <hip/hip_runtime.h>

#include "bpla_fast.h"
#include "launch.h"

namespace sk {

namespace {

constexpr int kNA = kAaSlots - 1;  // 23 letters

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A lane's current x row and the score of a cell of that row.
// cell(b, beta, sc, bs): sc = LAScore(x row, y column b), bs = exp(beta * sc).
struct CodeScore {
  const double* ft;  // exp(beta * t), [y residue][x residue]
  const double* st;  // t
  const uint8_t* xcode;
  const uint8_t* ycode;  // LDS
  int xa;
  __device__ __forceinline__ void clear() { xa = kNA; }
  __device__ __forceinline__ void load_row(int row) { xa = xcode[row - 1]; }  // 1-based, <= Lx
  __device__ __forceinline__ void cell(int b, double, double& sc, double& bs) const {
    const int k = (int)ycode[b - 1] * kAaSlots + xa;
    sc = st[k];
    bs = ft[k];
  }
};

struct ProfScore {
  const double* tb;  // [x letter][y letter], zero padded to 24 x 24
  const float* xprof;
  const float* ycol;  // LDS: [column][24], slot 23 = the column's sum over the letters
  double u[kNA];
  float xs;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int l = 0; l < kNA; ++l) u[l] = 0.0;
    xs = 0.0f;
  }
  __device__ __forceinline__ void load_row(int row) {
    clear();
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
  }
  __device__ __forceinline__ void cell(int b, double beta, double& sc, double& bs) const {
    const float* yc = ycol + (b - 1) * kAaSlots;
    double v = 0.0;
#pragma unroll
    for (int l = 0; l < kNA; ++l) v = __builtin_fma(u[l], (double)yc[l], v);
    const float n = xs * yc[kNA];
    sc = n == 0.0f ? 0.0 : v / (double)n;
    bs = exp(beta * sc);
  }
};

// One pair on one wave: value and d/d(beta, gap, ext) in every lane.
template <class Score>
__device__ __forceinline__ void la_grad_pair(Score& S, const LaProtGradLaunch& P, int Lx, int Ly, double* bnd,
                                             double* __restrict__ Bt, int lane, double& value, double (&g)[3]) {
  const double beta = P.beta, gap = P.gap, ext = P.ext;
  const double bg = P.beta_gap, be = P.beta_ext;
  const int Lys = max(Ly, 64);
  const int T = bpla_steps(Lx, Ly);
  const int64_t TS = (int64_t)T * 64;
  double* __restrict__ BM = Bt;
  double* __restrict__ BX = Bt + TS;
  double* __restrict__ BY = Bt + 2 * TS;

  // ---------------------------------------------------------------- backward
  double* bndX = bnd;              // B_IX of row 64s+1 (lane 0), column b
  double* bndP = bnd + (Lys + 2);  // bs * B_M of the same cells
  for (int j = lane; j < 2 * (Lys + 2); j += 64) bnd[j] = 0.0;
  wave_sync();
  {
    double oX = 0.0, oP = 0.0, oY = 0.0;  // my outputs of the previous (reverse) step
    double dP = 0.0;                      // P(a+1, b+1): received a step earlier
    int s_cur = -1;
    S.clear();
    // the lane's cell at step t: u = t - lane, strip s = u / Lys, column
    // b = u % Lys + 1 (u < 0: s = -1, idle), counted down from the last step
    const int u0 = T - 1 - lane;
    int s = u0 >= 0 ? u0 / Lys : -1;
    int b = u0 - s * Lys + 2;
    for (int t = T - 1; t >= 0; --t) {
      if (--b < 1) {
        b = Lys;
        --s;
      }
      const int a = 64 * s + lane + 1;
      // lane 63's row a+1 is lane 0 of the next strip (boundary row)
      const int b63 = __builtin_amdgcn_readlane(b, 63);
      const int bi = (b63 >= 1 && b63 <= Ly) ? b63 : 0;
      const double rX = wave_shl1_to(oX, bndX[bi]);
      const double rP = wave_shl1_to(oP, bndP[bi]);
      double M = 0.0, X = 0.0, Y = 0.0, Pn = 0.0;
      if (s >= 0 && b <= Ly && a <= Lx) {
        if (s != s_cur) {
          S.load_row(a);
          s_cur = s;
        }
        const bool an = a < Lx, bm = b < Ly;
        const double diag = (an && bm) ? dP : 0.0;
        const double iyr = bm ? oY : 0.0;
        const double ixd = an ? rX : 0.0;
        M = diag + (an ? __builtin_fma(bg, ixd, 1.0) : 0.0) + (bm ? __builtin_fma(bg, iyr, a == Lx ? 1.0 : 0.0) : 0.0);
        X = diag + (an ? be * ixd : 0.0) + (bm ? bg * iyr : 0.0);
        Y = diag + (bm ? be * iyr : 0.0);
        if (!an && !bm) {  // (n, m): B_M = B_RX = B_RY = 1
          M = 1.0;
          X = Y = 0.0;
        }
        double sc, bs;
        S.cell(b, beta, sc, bs);
        Pn = bs * M;
        BM[(int64_t)t * 64 + lane] = M;
        BX[(int64_t)t * 64 + lane] = X;
        BY[(int64_t)t * 64 + lane] = Y;
        if (lane == 0) {
          bndX[b] = X;
          bndP[b] = Pn;
        }
      }
      oX = X;
      oP = Pn;
      oY = Y;
      dP = rP;
    }
  }
  wave_sync();

  // ---------------------------------------------------------------- forward + gradients
  for (int j = lane; j < 3 * (Lys + 1); j += 64) bnd[j] = 0.0;  // row 0 (M, IX, IY)
  wave_sync();
  int j = 1 - lane, i = lane + 1;
  bool row_ok = i <= Lx;
  S.clear();
  if (row_ok) S.load_row(i);
  double lM = 0.0, lX = 0.0, lY = 0.0;  // (i, j-1)
  double dM = 0.0, dX = 0.0, dY = 0.0;  // (i-1, j-1): received a step earlier
  double acc = 0.0, gb = 0.0, gg = 0.0, ge = 0.0;
  // B at (step t, lane), fetched a step ahead
  double nbm = T > 0 ? BM[lane] : 0.0, nbx = T > 0 ? BX[lane] : 0.0, nby = T > 0 ? BY[lane] : 0.0;
  for (int t = 0; t < T; ++t) {
    const double bm = nbm, bx = nbx, by = nby;
    if (t + 1 < T) {
      nbm = BM[(int64_t)(t + 1) * 64 + lane];
      nbx = BX[(int64_t)(t + 1) * 64 + lane];
      nby = BY[(int64_t)(t + 1) * 64 + lane];
    }
    const int jb = __builtin_amdgcn_readfirstlane(j);
    const double* bj = bnd + 3 * (jb >= 1 && jb <= Ly ? jb : 0);
    const double uM = wave_shr1(lM, bj[0]);
    const double uX = wave_shr1(lX, bj[1]);
    const double uY = wave_shr1(lY, bj[2]);
    if (j >= 1 && j <= Ly && row_ok) {
      double sc, bs;
      S.cell(j, beta, sc, bs);
      const bool c1 = j == 1;
      // F_M + F_IX + F_IY + F_LX + F_LY at (i-1, j-1): F_LX = 1 and F_LY = j
      // on rows >= 1; row 0 holds F_M = F_LX = F_LY = 1 at (0, 0), F_LY = 1
      const double extra = i == 1 ? (c1 ? 3.0 : 1.0) : (double)j;
      const double nM = bs * (dM + dX + dY + extra);
      const double nX = bg * uM + be * uX;
      const double lMX = c1 ? 0.0 : lM + lX, lYc = c1 ? 0.0 : lY;
      const double nY = bg * lMX + be * lYc;
      acc += nM;
      const double vd = nM * bm;
      const double vgx = uM * bg * bx, vex = uX * be * bx;
      const double vgy = lMX * bg * by, vey = lYc * be * by;
      gb += sc * vd + gap * (vgx + vgy) + ext * (vex + vey);
      gg += beta * (vgx + vgy);
      ge += beta * (vex + vey);
      lM = nM;
      lX = nX;
      lY = nY;
      if (lane == 63) {
        double* bw = bnd + 3 * j;
        bw[0] = nM;
        bw[1] = nX;
        bw[2] = nY;
      }
    }
    dM = uM;
    dX = uX;
    dY = uY;
    if (++j > Lys) {  // next strip: row i + 64, column 1
      j = 1;
      i += 64;
      row_ok = i <= Lx;
      if (row_ok) S.load_row(i);
      dM = dX = dY = 0.0;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_xor(acc, off, 64);
    gb += __shfl_xor(gb, off, 64);
    gg += __shfl_xor(gg, off, 64);
    ge += __shfl_xor(ge, off, 64);
  }
  value = 1.0 + acc;
  g[0] = gb;
  g[1] = gg;
  g[2] = ge;
  wave_sync();
}

}  // namespace

template <bool PROF>
__global__ void __launch_bounds__(256) sk_la_prot_grad_kernel(LaProtGradLaunch P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int maxlen = P.lds_max_len;  // even
  // LDS: code: factors [24 y][24 x] | scores [24 y][24 x]; profile: table [24 x][24 y]
  //      | per wave: boundary rows 3 x [maxlen + 2] | y codes [maxlen] or y columns [maxlen][24] float
  double* tb0 = reinterpret_cast<double*>(smem);
  double* tb1 = tb0 + kAaSlots * kAaSlots;
  unsigned char* wbase = smem + (PROF ? 1 : 2) * kAaSlots * kAaSlots * 8 +
                         (size_t)wave * (PROF ? la_prot_grad_prof_wave_lds_bytes(maxlen)
                                              : la_prot_grad_code_wave_lds_bytes(maxlen));
  double* bnd = reinterpret_cast<double*>(wbase);
  unsigned char* ybase = wbase + (size_t)3 * (maxlen + 2) * 8;
  for (int k = threadIdx.x; k < kAaSlots * kAaSlots; k += blockDim.x) {
    const int r = k / kAaSlots, c = k - r * kAaSlots;
    if (PROF) {  // r: x letter, c: y letter
      tb0[k] = r < kNA && c < kNA ? P.table[r * kNA + c] : 0.0;
    } else {  // r: y residue, c: x residue
      const double t = r < kNA && c < kNA ? P.table[c * kNA + r] : 0.0;
      tb0[k] = r < kNA && c < kNA ? exp(P.beta * t) : 1.0;
      tb1[k] = t;
    }
  }
  __syncthreads();
  double* Bt = P.scratch + (int64_t)(blockIdx.x * (blockDim.x >> 6) + wave) * P.bt_doubles;
  auto next_pair = [&]() {
    unsigned long long v = 0;
    if (lane == 0) v = atomicAdd(P.pair_counter, 1ull);
    return (int64_t)(((unsigned long long)__builtin_amdgcn_readlane((unsigned)(v >> 32), 0) << 32) |
                     (unsigned)__builtin_amdgcn_readlane((unsigned)v, 0));
  };
  for (int64_t pr = next_pair(); pr < P.n_pairs; pr = next_pair()) {
    const int x = __builtin_amdgcn_readfirstlane(P.xs[pr]);
    const int y = __builtin_amdgcn_readfirstlane(P.ys[pr]);
    const int Lx = __builtin_amdgcn_readfirstlane(P.xset.ex_len[x]);
    const int Ly = __builtin_amdgcn_readfirstlane(P.yset.ex_len[y]);
    const int xpb = __builtin_amdgcn_readfirstlane(P.xset.ex_pos_base[x]);
    const int ypb = __builtin_amdgcn_readfirstlane(P.yset.ex_pos_base[y]);
    double v, g[3];
    if constexpr (PROF) {
      float* ycol = reinterpret_cast<float*>(ybase);
      const float* yprof = P.yset.prof + (size_t)ypb * kAaSlots;
      for (int k = lane; k < Ly * kAaSlots; k += 64) ycol[k] = yprof[k];
      wave_sync();
      for (int j = lane; j < Ly; j += 64) {  // slot 23 := the column's sum over the letters
        float s = 0.0f;
        for (int l = 0; l < kNA; ++l) s += ycol[j * kAaSlots + l];
        ycol[j * kAaSlots + kNA] = s;
      }
      wave_sync();
      ProfScore S;
      S.tb = tb0;
      S.xprof = P.xset.prof + (size_t)xpb * kAaSlots;
      S.ycol = ycol;
      la_grad_pair(S, P, Lx, Ly, bnd, Bt, lane, v, g);
    } else {
      uint8_t* ycode = ybase;
      const uint8_t* yg = P.yset.code + ypb;
      for (int j = lane; j < Ly; j += 64) ycode[j] = yg[j];
      wave_sync();
      CodeScore S;
      S.ft = tb0;
      S.st = tb1;
      S.xcode = P.xset.code + xpb;
      S.ycode = ycode;
      la_grad_pair(S, P, Lx, Ly, bnd, Bt, lane, v, g);
    }
    if (lane == 0) {
      const int64_t o = P.oidx ? P.oidx[pr] : pr;
      P.value[o] = v;
      P.grad[4 * o + 0] = 0.0;  // d/d alpha: w_pair = 0
      P.grad[4 * o + 1] = g[0];
      P.grad[4 * o + 2] = g[1];
      P.grad[4 * o + 3] = g[2];
    }
  }
}

static hipError_t la_grad_launch(const void* fn, const LaProtGradLaunch& P, int grid, int nwaves, size_t lds,
                                 hipStream_t st) {
  if (P.n_pairs == 0 || grid <= 0) return hipSuccess;
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  LaProtGradLaunch a = P;
  void* args[] = {&a};
  return hipLaunchKernel(fn, dim3(grid), dim3(64 * nwaves), args, lds, st);
}

hipError_t launch_la_prot_grad_code(const LaProtGradLaunch& P, int grid, int nwaves, hipStream_t st) {
  return la_grad_launch(reinterpret_cast<const void*>(sk_la_prot_grad_kernel<false>), P, grid, nwaves,
                        la_prot_grad_code_lds_bytes(P.lds_max_len, nwaves), st);
}

hipError_t launch_la_prot_grad_prof(const LaProtGradLaunch& P, int grid, int nwaves, hipStream_t st) {
  return la_grad_launch(reinterpret_cast<const void*>(sk_la_prot_grad_kernel<true>), P, grid, nwaves,
                        la_prot_grad_prof_lds_bytes(P.lds_max_len, nwaves), st);
}

}  // namespace sk
