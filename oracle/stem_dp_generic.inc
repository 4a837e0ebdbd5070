/* stem_dp_generic.inc -- stem_dp (sk_oracle.c) over a caller's gap-weight
 * table, in the arithmetic type REAL.  Included by sk_oracle.c once per type
 * with REAL and SUFFIX(name) defined.  TEST INFRASTRUCTURE ONLY.
 *
 * The tables are those of stem_dp: co_subst from the double exp, the float
 * bpfreq and node weights, the caller's double w[k] where stem_dp reads
 * loop_gap^k, and gap2 where it reads loop_gap * loop_gap.  Only the DP's
 * products and sums are formed in REAL, in stem_dp's order: with REAL =
 * double, w[k] = gap_powers(loop_gap)[k] and gap2 = loop_gap * loop_gap every
 * operation is stem_dp's own.  A gap beyond the table (>= nw) gives NaN. */

static REAL SUFFIX(node_gap)(double gap2, const orc_mdata *d, int i) {
  return (REAL)gap2 * d->tree[i].weight;
}

static REAL SUFFIX(node_match)(const stem_params *S, double gap2, const orc_mdata *x,
                               const orc_mdata *y, int i, int j) {
  const onode *ni = &x->tree[i], *nj = &y->tree[j];
  REAL v_c = 0.0;
  for (int a = 0; a != ni->n_bpf; ++a) {
    REAL cx = ni->bpf[a].p;
    for (int b = 0; b != nj->n_bpf; ++b) {
      REAL cy = nj->bpf[b].p;
      REAL v;
      if (S->subst) {
        v = S->co_subst[ni->bpf[a].code * 16 + nj->bpf[b].code];
      } else {
        v = (ni->bpf[a].code != nj->bpf[b].code) ? S->mismatch : S->match;
      }
      v_c += v * cx * cy;
    }
  }
  REAL nbp_x = x->prof5[ni->first * 5 + RNA_GAP];
  v_c += SUFFIX(node_gap)(gap2, y, j) * nbp_x / (REAL)x->n_seqs;
  REAL nbp_y = y->prof5[nj->first * 5 + RNA_GAP];
  v_c += SUFFIX(node_gap)(gap2, x, i) * nbp_y / (REAL)y->n_seqs;
  return v_c;
}

static double SUFFIX(stem_dp_tab)(const stem_params *S, const double *w, int nw, double gap2,
                                  const orc_mdata *x, const orc_mdata *y) {
  int nx = x->n_nodes, ny = y->n_nodes;
  for (int s = 0; s != 2; ++s) {
    const orc_mdata *d = s ? y : x;
    for (int i = 0; i != d->n_nodes; ++i)
      for (int e = 0; e != d->tree[i].n_edges; ++e)
        if (d->tree[i].edges[e].gaps >= (uint32_t)nw) return NAN;
  }
  size_t cells = (size_t)(nx ? nx : 1) * (ny ? ny : 1);
  REAL *K0 = (REAL *)malloc(sizeof(REAL) * cells);
  REAL *G0 = (REAL *)malloc(sizeof(REAL) * cells);
  REAL *K1 = (REAL *)calloc(ny ? ny : 1, sizeof(REAL));
  REAL *G1 = (REAL *)calloc(ny ? ny : 1, sizeof(REAL));
#define AT(M, a, b) M[(size_t)(a) * ny + (b)]
  for (int i = 0; i != nx; ++i) {
    const onode *xi = &x->tree[i];
    for (int j = 0; j != ny; ++j) {
      const onode *yj = &y->tree[j];
      if (xi->n_edges == 0 && yj->n_edges == 0) {
        AT(K0, i, j) = AT(G0, i, j) = 1.0;
        continue;
      }
      K1[j] = G1[j] = 0.0;
      if (xi->n_edges && yj->n_edges &&
          (S->band == 0 ||
           (unsigned)abs((int)((xi->last - xi->first) - (yj->last - yj->first))) <= S->band)) {
        REAL v_s = SUFFIX(node_match)(S, gap2, x, y, i, j);
        for (int ex = 0; ex != xi->n_edges; ++ex) {
          for (int ey = 0; ey != yj->n_edges; ++ey) {
            REAL e_s = (REAL)w[xi->edges[ex].gaps] * w[yj->edges[ey].gaps] * 1.0f * 1.0f;
            REAL v = AT(G0, xi->edges[ex].to, yj->edges[ey].to) * v_s * e_s;
            K1[j] += v;
            G1[j] += v;
          }
        }
      }
      for (int ey = 0; ey != yj->n_edges; ++ey) {
        REAL v_s = SUFFIX(node_gap)(gap2, y, j);
        REAL e_s = (REAL)w[yj->edges[ey].gaps] * 1.0f;
        K1[j] += K1[yj->edges[ey].to];
        G1[j] += G1[yj->edges[ey].to] * v_s * e_s;
      }
      AT(K0, i, j) = K1[j];
      AT(G0, i, j) = G1[j];
      for (int ex = 0; ex != xi->n_edges; ++ex) {
        REAL v_s = SUFFIX(node_gap)(gap2, x, i);
        REAL e_s = (REAL)w[xi->edges[ex].gaps] * 1.0f;
        AT(K0, i, j) += AT(K0, xi->edges[ex].to, j);
        AT(G0, i, j) += AT(G0, xi->edges[ex].to, j) * v_s * e_s;
      }
    }
  }
  REAL ret = 0.0;
  for (int a = 0; a != x->n_root; ++a)
    for (int b = 0; b != y->n_root; ++b) ret += AT(K0, x->root[a], y->root[b]);
#undef AT
  free(K0);
  free(G0);
  free(K1);
  free(G1);
  return (double)ret; /* the one rounding to double */
}
