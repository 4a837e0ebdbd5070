"""Fixtures, references and the error bound of the DAG stem kernels' long-gap
tests (tests/test_stem_long_gaps.py, tests/test_stem_visibility_cpu.py,
tests/test_stem_oracle_twin.py and the loop_gap 0.98 cases of the shared-path
tests).  DESIGN.md §7.1.

Every stem term carries loop_gap^(gaps_x + gaps_y); at the loop_gap 0.2-0.6 of
the older tests an edge that skips more than a dozen positions is below their
tolerance.  The cases here use loop_gap 0.98 (L <= 420), 0.999 (L = 1,100)
and 1.0, so that every edge and the length band reach the compared digits,
and a tolerance derived from the roundings of the DP (rounding_depth) instead
of 1e-6.  References: the long-double twin of the oracle's stem_dp
(oracle/stem_dp_generic.inc), live for L <= 120 and from
tests/golden/stem_long_gaps.npz (make_golden_long_gaps.py) above.
"""
import functools
import math
import os

import numpy as np

import stem_kernel_amd as ska
from oracle import pyoracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53
TOL_CAP = 1e-11       # no fixture's stem tolerance may exceed this
STR_TOL = 1e-6        # the profile string kernel's bound in this suite (tests/test_gpu_parity.py), not derived here
SEED = 0x57E30
LONG_GAP = 0.98      # the shared-path tests' long-gap cases and the class sets
# (loop_gap, len_band): bands off / default / wide at 0.98; the boundary 1.0 with the band off (where every
# bucket is visible, tests/test_stem_visibility_cpu.py) and at the default band
PARAMS = [(0.98, 0), (0.98, 10), (0.98, 30), (1.0, 0), (1.0, 10)]
GAP_PARAMS = [(0.999, 0), (0.999, 10), (0.999, 30), (1.0, 0), (1.0, 10)]   # the L = 1,100 gap-field cases
KINDS = (0, 1, 4, 5, 6, 7)
STEM_KINDS = (0, 1, 6)   # where K_str outweighs the stem part by more than 1 / STR_TOL, kinds 4, 5, 7 see no stem
BUCKETS = [(13, 32), (33, 128), (129, 1023), (1024, 1 << 30)]


# ------------------------------------------------------------------ the bound
def dag_stats(dag) -> dict:
    """Per DAG (oracle or product layout: n_edges, edge_to node-major, roots,
    n_bpfreq): H the depth (edges on the longest root-to-leaf chain), E the
    largest edge count of a node, B the largest bpfreq count, R the root
    count, and over every descending chain the largest sum of edge counts (P)
    and of squared edge counts (Q)."""
    ne = np.asarray(dag["n_edges"], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(ne)])
    to = np.asarray(dag["edge_to"], dtype=np.int64)
    n = len(ne)
    h, p, q = (np.zeros(n, np.int64) for _ in range(3))
    for i in range(n):  # children are built before their parents
        if ne[i]:
            c = to[off[i]:off[i + 1]]
            assert c.max() < i
            h[i], p[i], q[i] = 1 + h[c].max(), ne[i] + p[c].max(), ne[i] ** 2 + q[c].max()
    r = np.asarray(dag["roots"], dtype=np.int64)
    top = lambda a: int(a[r].max()) if len(r) else 0
    gaps = np.asarray(dag["edge_gaps"])
    return dict(H=top(h), P=top(p), Q=top(q), E=int(ne.max()) if n else 0,
                B=int(np.max(dag["n_bpfreq"])) if n else 0, R=len(r),
                nl=int(np.sum(ne > 0)), gmax=int(gaps.max()) if len(gaps) else 0)


def _ceil_sqrt(q: int) -> int:
    r = math.isqrt(q)
    return r if r * r == q else r + 1


def rounding_depth(sx: dict, sy: dict) -> int:
    """D: a bound on the roundings along any chain of double operations that
    feeds K(x, y) in stem_dp (oracle/sk_oracle.c), the tables (co_subst, gap
    powers, bpfreq, weights) taken as given.  All terms are positive, so the
    double result is within D * 2^-53 (to first order) of the exact value of
    the same tables, in this and in any other order of the same sums.

    A chain runs from a root cell (i, j) down to a leaf cell; each step takes
    it to a child in x, in y or in both, so it has at most Hx + Hy steps.

    * products per step, at most Bx*By + 8: a step in both takes the node
      match score (Bx*By terms of two products, two gap terms of three, summed:
      at most Bx*By + 4 roundings), the edge score g[a]*g[b] (1) and two
      products with G0 (2); a step in x or y alone takes gap2*weight and two
      products (3).
    * sums: the term of a both-step is added into a sum of e_i*e_j match
      terms, then e_j y-gap terms, then e_i x-gap terms; of a y-step, into at
      most e_j + e_i; of an x-step, into at most e_i (e: edge count of the
      parent).  The x nodes of the steps that move in x are distinct nodes of
      one descending chain, likewise in y, so over a chain
        sum e_i*e_j <= sqrt(Qx*Qy)   (Cauchy-Schwarz),
        sum e_i     <= Px + Ex*Hy,   sum e_j <= Py + Ey*Hx
      (stem_dp's x-steps enter sums of e_i only, so Ey*Hx is slack there;
      it is kept so that D is the same with the roles of x and y exchanged,
      as in a kernel that runs its loops the other way round).
    * the Rx*Ry root cells are summed at the end.

      D = (Bx*By + 8)*(Hx + Hy) + Px + Py + Ex*Hy + Ey*Hx
          + ceil(sqrt(Qx*Qy)) + Rx*Ry
    """
    return ((sx["B"] * sy["B"] + 8) * (sx["H"] + sy["H"]) + sx["P"] + sy["P"] + sx["E"] * sy["H"]
            + sy["E"] * sx["H"] + _ceil_sqrt(sx["Q"] * sy["Q"]) + sx["R"] * sy["R"])


def stem_tol(sx: dict, sy: dict) -> float:
    """Relative tolerance of a GPU stem value against the long-double
    reference: 4 * D * 2^-53.  The factor 4 covers the kernel's factorings
    (closed forms, Gamma / Phi tables, shared sums), which distribute and
    reassociate the same positive terms, and the reference's own rounding."""
    return 4.0 * rounding_depth(sx, sy) * U


def tol_matrix(stats_x, stats_y=None) -> np.ndarray:
    stats_y = stats_x if stats_y is None else stats_y
    return np.array([[stem_tol(a, b) for b in stats_y] for a in stats_x])


def maxk(nl: int) -> int:
    """Register class of a y with nl non-leaf nodes (tests/test_large_configs.py)."""
    s = (nl + 1 + 63) // 64
    return 17 if s == 17 else (s + 3) // 4 * 4


# ------------------------------------------------------------------ the inputs
def _om(seq):
    return po.OMData([seq], [ska.fold(seq.lower())], 0.01)


def _by_class(seqs, classes):
    """The first sequence of each wanted class, by its non-leaf node count."""
    k = [maxk(dag_stats(_om(s).dag())["nl"]) for s in seqs]
    pick = []
    for c in classes:
        pick.append(next(i for i in range(len(seqs)) if k[i] == c and i not in pick))
    return [seqs[i] for i in pick]


def _fewest_roots(seqs, classes):
    """Per wanted class the sequence with the fewest DAG roots (the root sum
    is the largest part of D at L = 400), one more for a repeated class."""
    st = [dag_stats(_om(s).dag()) for s in seqs]
    order = sorted(range(len(seqs)), key=lambda i: (st[i]["R"], i))
    pick = []
    for c in classes:
        pick.append(next(i for i in order if maxk(st[i]["nl"]) == c and i not in pick))
    return [seqs[i] for i in pick]


# name -> (register classes that must run, uses the golden file)
CLASS_SETS = {"L40": ({4}, False), "L60": ({8}, False), "L120": ({12, 16}, False),
              "L200": ({16, 17, 20}, True), "L300": ({24}, True), "L400": ({28, 32}, True)}


@functools.lru_cache(maxsize=None)
def class_set(name):
    """Three single sequences per length, picked by node count so that the
    register classes MAXK 4, 8, 12, 16, 17, 20, 24 (and 28, 32) all run."""
    if name in ("L40", "L60", "L120"):
        L = int(name[1:])
        return tuple(ska.random_sequences(3, L, SEED + L))
    dag = np.load(os.path.join(GOLDEN, "large_dag.npz"))
    if name == "L200":
        seqs = [str(s) for n in ("ns_L200", "ns20_L200") for s in dag[f"{n}_seqs"]]
        return tuple(_by_class(seqs, (16, 17, 20)))
    if name == "L300":
        return tuple(str(s) for s in dag["c5_L300_seqs"][:3])
    if name == "L400":
        return tuple(_fewest_roots(ska.random_sequences(24, 400, SEED + 400), (28, 28, 32)))
    raise KeyError(name)


def gap_example(G, seed, L=1100):
    """(sequence, packed bpp) of L = 1,100 whose largest edge gap is exactly
    G: the pair (1, L) over the pair (501, L + 498 - G) (1-based, p = 0.5
    each) and a short helix inside, as make_golden_big.py::gap_case."""
    seq = ska.random_sequences(1, L, seed)[0]
    bpp = np.zeros(L * (L - 1) // 2)

    def put(i, j, p):  # 0-based i < j, row-major upper triangle without diagonal
        bpp[i * L - i * (i + 1) // 2 + (j - i - 1)] = p
    put(0, L - 1, 0.5)
    put(500, L + 497 - G, 0.5)
    for k in range(4):
        put(502 + k, 518 - k, 0.3)
    return seq, bpp


GAP_EDGES = (1022, 1023, 1024, 1077)


@functools.lru_cache(maxsize=None)
def gap_set():
    """[(rows, bpps)]: the four gap examples and one folded L = 60 sequence."""
    items = [gap_example(G, SEED + G) for G in GAP_EDGES]
    s60 = ska.random_sequences(1, 60, SEED + 61)[0]
    return tuple(items) + ((s60, ska.fold(s60.lower())),)


def table_end_example(L=90):
    """One pair (2, L - 1) (1-based): its hairpin edge skips L - 4 positions,
    the largest index a DAG of this length reads in the gap-power table but
    for the single outermost pair."""
    seq = ska.random_sequences(1, L, SEED + 90)[0]
    bpp = np.zeros(L * (L - 1) // 2)
    bpp[1 * L - 1 + (L - 2 - 1 - 1)] = 0.6
    return seq, bpp


def build(items):
    """(Dataset, [OMData]) of [(sequence, packed bpp)] or plain sequences."""
    ds, om = ska.Dataset(), []
    for k, it in enumerate(items):
        seq, bpp = (it, ska.fold(it.lower())) if isinstance(it, str) else it
        ds.add("+1" if k % 2 == 0 else "-1", [seq], [bpp], th=0.01, use_bp=True)
        om.append(po.OMData([seq], [bpp], 0.01))
    return ds, om


# ------------------------------------------------------------------ references
def _key(name, g, band, what):
    return f"{name}_g{g}_b{band}_{what}"


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "stem_long_gaps.npz"))


def ld_matrices(om_x, om_y, g, band, kern_su=None, kern_si=None):
    """(su, si)[x, y] by the long-double twin at the kernels' default scores."""
    ps, pi = (kern_su or ska.SuStemKernel()).params, (kern_si or ska.SiStemKernel()).params
    su = np.array([[po.su_stem_ld(a, b, g, ps.beta, band) for b in om_y] for a in om_x])
    si = np.array([[po.si_stem_ld(a, b, g, pi.stack, pi.covar, band) for b in om_y] for a in om_x])
    return su, si


def str_matrices(om_x, om_y):
    p = ska.SiStemStrKernel().params
    k2 = np.array([[po.su_str(a, b, p.gap, ska.SuStemStrKernel().params.alpha) for b in om_y] for a in om_x])
    k3 = np.array([[po.si_str(a, b, p.gap, p.match, p.mismatch) for b in om_y] for a in om_x])
    return k2, k3


@functools.lru_cache(maxsize=None)
def built(name):
    """(Dataset, [OMData], [dag_stats]) of a class set or of the gap set."""
    ds, om = build(gap_set() if name == "gap" else class_set(name))
    return ds, om, [dag_stats(o.dag()) for o in om]


@functools.lru_cache(maxsize=None)
def reference(name, g, band):
    """dict su, si (long double, rounded once), k2, k3 (string parts), all
    [x, y] over the set, read-only: from the golden file where the set uses
    it, else live."""
    if name == "gap" or CLASS_SETS[name][1]:
        z = golden()
        r = {w: z[_key(name, g, band, w)] for w in ("su", "si")}
        r["k2"], r["k3"] = z[f"{name}_k2"], z[f"{name}_k3"]
    else:
        _, om, _ = built(name)
        su, si = ld_matrices(om, om, g, band)
        k2, k3 = str_matrices(om, om)
        r = dict(su=su, si=si, k2=k2, k3=k3)
    for a in r.values():
        a.setflags(write=False)
    return r


def kernel(kind, g, band):
    return {0: ska.SuStemKernel, 1: ska.SiStemKernel, 4: ska.SuStemStrKernel, 5: ska.SiStemStrKernel,
            6: ska.LSuStemKernel, 7: ska.LSuStemStrKernel}[kind](loop_gap=g, len_band=band)


def excess(kind, got, ref, tol, p):
    """max over the entries of |got - expected| / allowed for one kind: the
    stem part within tol (relative), the string part of kinds 4, 5 and 7
    within STR_TOL; kinds 6 and 7 on beta log K (+ alpha log K_str) with the
    absolute tolerance |beta| tol (+ |alpha| STR_TOL) plus 4 ulp of the
    result."""
    su, si, k2, k3 = ref["su"], ref["si"], ref["k2"], ref["k3"]
    if kind in (0, 1):
        exp = su if kind == 0 else si
        allowed = tol * exp
    elif kind in (4, 5):
        stem, s = (su, k2) if kind == 4 else (si, k3)
        exp = stem + s
        allowed = tol * stem + STR_TOL * s + 4 * np.spacing(exp)
    elif kind == 6:
        exp = p.beta * np.log(su)
        allowed = abs(p.beta) * tol + 4 * np.spacing(np.abs(exp))
    else:
        exp = p.beta * np.log(su) + p.alpha * np.log(k2)
        allowed = abs(p.beta) * tol + abs(p.alpha) * STR_TOL + 4 * np.spacing(np.abs(exp))
    return float(np.max(np.abs(np.asarray(got) - exp) / allowed)), float(np.max(np.abs(got - exp) / np.abs(exp)))


def su_excess(got, om_x, om_y, kern, upper=False):
    """SuStemKernel values got[x, y] against the live long-double twin:
    (max error / tolerance, max relative error, largest tolerance); upper:
    only x <= y (a Gram)."""
    p = kern.params
    sx = [dag_stats(o.dag()) for o in om_x]
    sy = sx if om_y is om_x else [dag_stats(o.dag()) for o in om_y]
    got = np.asarray(got, dtype=np.float64).reshape(len(om_x), len(om_y))
    worst = rel = top = 0.0
    for i, a in enumerate(om_x):
        for j, b in enumerate(om_y):
            if upper and j < i:
                continue
            ref = po.su_stem_ld(a, b, p.loop_gap, p.beta, p.len_band)
            tol = stem_tol(sx[i], sy[j])
            err = abs(got[i, j] - ref) / ref
            worst, rel, top = max(worst, err / tol), max(rel, err), max(top, tol)
    return worst, rel, top


# ------------------------------------------------------------------ visibility
def masked_change(x, y, g, band, lo, hi, n, score="su"):
    """Relative change of K(x, y) (double oracle, table variant) when the gap
    weights w[lo..hi] are zeroed."""
    w = po.gap_weights(g, n)
    f = po.su_stem_tab if score == "su" else po.si_stem_tab
    full = f(x, y, w, g * g, band=band)
    w[lo:min(hi, n - 1) + 1] = 0.0
    return abs(f(x, y, w, g * g, band=band) - full) / full


def band_change(x, y, g, band, score="su"):
    """Relative change of K(x, y) between len_band = band and the band off."""
    f = po.su_stem if score == "su" else po.si_stem
    off = f(x, y, g, band=0)
    return abs(f(x, y, g, band=band) - off) / off
