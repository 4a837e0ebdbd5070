/* stem4d_generic.inc -- the 4-D stem kernel's full_dp and band-constrained
 * partial_dp (stem4d_full, orc_stem4d_partial of sk_oracle.c) in the
 * arithmetic type REAL.  Included by sk_oracle.c once per type with REAL and
 * SUFFIX(name) defined.  TEST INFRASTRUCTURE ONLY.
 *
 * One body serves both DPs: partial_dp over the constraints [0, |y|] for
 * every x position takes none of its boundary branches and is full_dp
 * operation for operation, so band == 0 runs it over the full range and
 * band > 0 over the -b band of orc_stem4d_band.  (-a constraints are not
 * restated here.)  The inputs are those of the pinned functions: the double
 * gap, stack and subst, the float base-pair probabilities; only the DP's
 * products and sums are formed in REAL, in the pinned functions' order, so
 * with REAL = double every operation is their own.  The double result is the
 * one rounding of the long-double instantiation.
 *
 * It keeps all eight states (K0..K3, G0..G3) of every plane of the two live
 * columns j - 1 and j, as the pinned functions do: 2 (|x| + 1) planes of
 * 8 (|y| + 1)(|y| + 2) / 2 REALs (|y| = 1,100 with |x| = 16: 2.6 GB in long
 * double).
 *
 * cut >= 0 emulates a truncated gap-power table in the two base terms, for
 * the visibility tests only: G0 = g^(l-k) of the (j, j) planes is 0 where
 * l - k > cut, and G0 = g^(j-i) of the diagonal cells (l, l) is 0 where
 * j - i > cut.  cut < 0 (the pinned behaviour) changes no operation. */

static double SUFFIX(stem4d_dp)(const char *x, const double *bpx, const char *y, const double *bpy,
                                double gap, double stack, double subst, float bp_bound, int model,
                                unsigned loop, unsigned band, int cut) {
  const int n = (int)strlen(x), m = (int)strlen(y);
  const double g = gap;
  bp4 BX = {x, bpx, n, model, loop}, BY = {y, bpy, m, model, loop};
  if (n == 0) return 1.0; /* K0(0,0,0,m) of the initialised plane (0,0) */
  unsigned *cl = (unsigned *)malloc(sizeof(unsigned) * (n + 1));
  unsigned *chh = (unsigned *)malloc(sizeof(unsigned) * (n + 1));
  if (band > 0) {
    orc_stem4d_band(n, m, band, cl, chh);
  } else {
    for (int i = 0; i <= n; ++i) cl[i] = 0, chh[i] = (unsigned)m;
  }
  REAL *gpw = (REAL *)malloc(sizeof(REAL) * (m + 1));
  gpw[0] = 1.0;
  for (int i = 1; i <= m; ++i) gpw[i] = gpw[i - 1] * g;
  const size_t cells = (size_t)(m + 1) * (m + 2) / 2;
  const size_t plane = cells * 8;
#define CELL(k, l) ((size_t)(l) * ((l) + 1) / 2 + (size_t)(k))
  REAL *col[2];
  col[0] = (REAL *)calloc((size_t)(n + 1) * plane, sizeof(REAL));
  col[1] = (REAL *)calloc((size_t)(n + 1) * plane, sizeof(REAL));
  REAL result = 0.0;
  for (int j = 0; j <= n; ++j) {
    REAL *cur = col[j & 1], *prv = col[(j + 1) & 1];
#define DP(C, s, i, k, l) ((C)[(size_t)(i) * plane + (size_t)(s) * cells + CELL(k, l)])
    memset(&cur[(size_t)j * plane], 0, plane * sizeof(REAL));
    for (size_t c = 0; c < cells; ++c) cur[(size_t)j * plane + S_K0 * cells + c] = 1.0;
    for (int l = 0; l <= m; ++l) {
      DP(cur, S_G0, j, l, l) = 1.0;
      for (int k = l - 1; k >= 0; --k) {
        DP(cur, S_G0, j, k, l) = DP(cur, S_G0, j, k + 1, l) * g;
        if (cut >= 0 && l - k > cut) DP(cur, S_G0, j, k, l) = 0.0;
      }
    }
    for (int i = j - 1; i >= 0; --i) {
      const float bp_ij = bp4_prob(&BX, i, j - 1);
      memset(&cur[(size_t)i * plane], 0, plane * sizeof(REAL));
      for (int l = (int)cl[j]; l <= (int)chh[j]; ++l) {
        DP(cur, S_K0, i, l, l) = 1.0;
        DP(cur, S_G0, i, l, l) = DP(cur, S_G0, i + 1, l, l) * g;
        if (cut >= 0 && j - i > cut) DP(cur, S_G0, i, l, l) = 0.0;
        if (l == 0) continue;
        const int kt = (l - 1) < (int)chh[i] ? (l - 1) : (int)chh[i];
        for (int k = kt; k >= (int)cl[i]; --k) {
          if (l <= (int)chh[j - 1]) {
            DP(cur, S_K0, i, k, l) = DP(prv, S_K0, i, k, l);
            DP(cur, S_G0, i, k, l) = DP(prv, S_G0, i, k, l) * g;
          } else {
            DP(cur, S_K0, i, k, l) = DP(prv, S_K0, i, k, chh[j - 1]);
            DP(cur, S_G0, i, k, l) = DP(prv, S_G0, i, k, chh[j - 1]) * g * g;
          }
          if (k >= (int)cl[i + 1]) {
            DP(cur, S_K1, i, k, l) = DP(cur, S_K1, i + 1, k, l);
            DP(cur, S_G1, i, k, l) = DP(cur, S_G1, i + 1, k, l) * g;
          } else {
            DP(cur, S_K1, i, k, l) = DP(cur, S_K1, i + 1, cl[i + 1], l);
            DP(cur, S_G1, i, k, l) = DP(cur, S_G1, i + 1, cl[i + 1], l) * g * g;
          }
          if (l - 1 >= (int)cl[j] || k == l - 1) {
            DP(cur, S_K2, i, k, l) = DP(cur, S_K2, i, k, l - 1);
            DP(cur, S_G2, i, k, l) = DP(cur, S_G2, i, k, l - 1) * g;
          } else {
            DP(cur, S_K2, i, k, l) = 0.0;
            DP(cur, S_G2, i, k, l) = 0.0;
            for (int ll = k; ll != l; ++ll) {
              DP(cur, S_K2, i, k, l) += DP(cur, S_K3, i, ll, ll);
              DP(cur, S_G2, i, k, l) += DP(cur, S_G3, i, ll, ll) * gpw[l - k];
            }
          }
          if (k + 1 <= (int)chh[i]) {
            DP(cur, S_K3, i, k, l) = DP(cur, S_K3, i, k + 1, l);
            DP(cur, S_G3, i, k, l) = DP(cur, S_G3, i, k + 1, l) * g;
          } else {
            DP(cur, S_K3, i, k, l) = DP(cur, S_K3, i, l, l);
            DP(cur, S_G3, i, k, l) = DP(cur, S_G3, i, l, l) * gpw[l - k];
          }
          if (bp_ij > bp_bound) {
            const float bp_kl = bp4_prob(&BY, k, l - 1);
            if (bp_kl > bp_bound) {
              const REAL g0 = DP(prv, S_G0, i + 1, k + 1, l - 1);
              if (x[i] == y[k] && x[j - 1] == y[l - 1]) {
                DP(cur, S_K3, i, k, l) += g0 * stack * bp_ij * bp_kl;
                DP(cur, S_G3, i, k, l) += g0;
              } else {
                DP(cur, S_K3, i, k, l) += g0 * stack * subst * bp_ij * bp_kl;
              }
            }
          }
          DP(cur, S_K2, i, k, l) += DP(cur, S_K3, i, k, l);
          DP(cur, S_G2, i, k, l) += DP(cur, S_G3, i, k, l);
          DP(cur, S_K1, i, k, l) += DP(cur, S_K2, i, k, l);
          DP(cur, S_G1, i, k, l) += DP(cur, S_G2, i, k, l);
          DP(cur, S_K0, i, k, l) += DP(cur, S_K1, i, k, l);
          DP(cur, S_G0, i, k, l) += DP(cur, S_G1, i, k, l);
        }
      }
    }
    if (j == n) result = DP(cur, S_K0, 0, 0, m);
#undef DP
  }
#undef CELL
  free(col[0]);
  free(col[1]);
  free(cl);
  free(chh);
  free(gpw);
  return (double)result; /* the one rounding to double */
}
