"""Fixtures, references and the error bound of the profile string kernels'
boundary and long-run tests (tests/test_string_long_gaps.py,
tests/test_string_visibility_cpu.py, tests/test_string_oracle_twin.py).
DESIGN.md §7.2.

The string DP (profile_string.hip; oracle/sk_oracle.c::orc_profile_string)

    v[i][j]  = G0[i-1][j-1] f[i][j]           f: weights x subst score
    K1[i][j] = v[i][j] + K1[i][j-1]           G1[i][j] = v[i][j] + G1[i][j-1] g
    K0[i][j] = K1[i][j] + K0[i-1][j]          G0[i][j] = G1[i][j] + G0[i-1][j] g
    K0[0][j] = K0[i][0] = 1, G0[0][j] = g^j, G0[i][0] = g^i,  K = K0[Lx][Ly]

on random sequences is dominated by dense alignments: a term that touches
G0[i][0] or G0[0][j] far from the corner, or that skips more than 64
positions in one run, is below 1e-18 of K even at g = 1.  The sparse probes
here have one or two non-zero cells f, so that K - 1 consists of exactly
those terms; the dense class sets run the kernels on realistic inputs at
g = 0.8, 0.98 and 1.  References: the long-double twins of the oracle's DPs
(orc_profile_string_ld, orc_naive_string_ld), live; the tolerance is derived
from the roundings of the DP (rounding_depth) instead of 1e-6.
"""
import functools

import numpy as np

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem_long_gaps as slg
from tests.helpers import mutate_alignment

U = 2.0 ** -53
TOL_CAP = 1e-11      # DESIGN §7.1's ceiling: no fixture's tolerance may exceed it
GAPS = (0.98, 0.999, 1.0)          # the sparse probes
DENSE_GAPS = (0.8, 0.98, 1.0)      # the dense class sets
# the dense sets' two score tables: exp(alpha ribosum) and match / mismatch (the kernel's defaults; K is at most
# 8.5e230 at L = 400, gap 1, unweighted, so neither had to be lowered)
ALPHA, MATCH, MISMATCH = 0.2, 1.0, 0.8
SUM_PARAMS = ((0.98, 0), (1.0, 10))  # (loop_gap, len_band) of kinds 4, 5 and 7

# Roundings of a cell's factor f against the twin's (a chain, not a count of operations: all terms are >= 0):
#   one-hot kernel  dG * w_x * w_y * st[c_x][c_y]: 3, in the oracle's order; the twin's factor is the same numbers
#   general kernel  dG * w_x * w_y * prof_subst: 3; prof_subst is the oracle's own, operation by operation
#   naive mode      dG * (g * g): 1; g * g as the oracle's
#   dyadic kernel   x role u / s * w with u a 4-term sum of products (1 + 3 + 1 + 1 = 6), y role c / s * w (2), the
#                   4-term FMA sum of their products (4) and dG * s (1): 13 against the exact factor; the twin's
#                   prof_subst is up to 18 from it (two products, 15 additions, the division; its float n is exact
#                   for these columns), so 31
F_PATH = dict(onehot=3, general=3, naive=1, dyadic=31)


# ------------------------------------------------------------------ the bound
def rounding_depth(lx: int, ly: int, path: str = "dyadic") -> int:
    """D: a bound on the roundings along any chain of double operations that
    feeds K0[Lx][Ly] in the recurrence above, the per-cell inputs (weights,
    prof_subst, the score table, g) taken as the double oracle computes them.
    Every term is >= 0 (scores exp(.) or match / mismatch >= 0, weights >= 0,
    g > 0), so any evaluation order in double lies within D * 2^-53 (to first
    order) of the exact value.

    A chain runs from K0[Lx][Ly] back to a boundary value through cells
    (i, j) -> (i-1, j) (K0 or G0 of the row above), (i, j-1) (K1 or G1 of the
    column before) or (i-1, j-1) (through v), so it visits at most Lx + Ly
    cells, and at most min(Lx, Ly) of its steps are diagonal.

    * in a cell it passes through at most K1 or G1 and K0 or G0: G1 = v +
      G1' g and G0 = G1 + G0' g round twice each (once if fused): at most 4
      per cell, 4 (Lx + Ly) in all -- one rounding each for K1, G1, K0 and
      G0 per step;
    * a diagonal step multiplies by the cell's factor: F roundings, F of the
      kernel that ran (F_PATH; the worst, the dyadic kernel's 31, where a
      call mixes them): F min(Lx, Ly);
    * the chain ends in G0[0][j] or G0[i][0], a repeated product g^k in the
      kernels' table (the twin's powers are long double): at most
      max(Lx, Ly) roundings;
    * the twin's own rounding to double: 1.

      D = 4 (Lx + Ly) + F min(Lx, Ly) + max(Lx, Ly) + 1
    """
    return 4 * (lx + ly) + F_PATH[path] * min(lx, ly) + max(lx, ly) + 1


def str_tol(lx, ly, path="dyadic") -> float:
    """Relative tolerance of a GPU string value against the long-double twin:
    4 * D * 2^-53, the 4 as in stem_long_gaps.stem_tol (FMA contractions and
    the kernels' factorings of the same non-negative terms)."""
    return 4.0 * rounding_depth(lx, ly, path) * U


def tol_matrix(len_x, len_y=None, path="dyadic") -> np.ndarray:
    len_y = len_x if len_y is None else len_y
    return np.array([[str_tol(a, b, path) for b in len_y] for a in len_x])


def gap_powers(g: float, n: int) -> np.ndarray:
    """g^k as the kernels and the double oracle form it: repeated products."""
    return po.gap_weights(g, n + 1)


# ------------------------------------------------------------------ LDS model
# launch.h / profile_string.hip / pairs_dag.cpp restated: the bytes the kernels take, from which the tests compute
# the y lengths where the launch shape changes (the shapes that ran are asserted through Context.last_string()).
LDS_WG, LDS_CU = 65536, 163840


def str_lds_bytes(max_len_y: int, nwaves: int) -> int:
    L = (max(max_len_y, 1) + 1) & ~1
    return 16 * 8 + nwaves * (2 * (L + 2) * 8 + L * 16 + L * 4 + L * 4)


def str_fast_wave_lds_bytes(max_len_y: int, onehot: bool) -> int:
    L = (max(max_len_y, 64) + 1) & ~1
    return (L * (8 if onehot else 32) + 2 * (L + 2) * 8 + 15) & ~15


def general_waves(max_len_y: int) -> int:
    """Waves per workgroup of the general kernel; 0: too long for its LDS."""
    w = 4
    while w > 1 and str_lds_bytes(max_len_y, w) > LDS_WG:
        w //= 2
    return w if str_lds_bytes(max_len_y, w) <= LDS_CU else 0


def fast_waves(max_len_y: int, onehot: bool) -> int:
    """Waves per workgroup of a fast kernel; 0: the call goes to the general
    kernel (the hand-over is by the dyadic kernel's rows for both)."""
    if str_fast_wave_lds_bytes(max_len_y, False) + 128 > LDS_CU:
        return 0
    return min(4, max(1, min(16, (LDS_CU - 128) // str_fast_wave_lds_bytes(max_len_y, onehot))))


def last_below(f, lo=1, hi=1 << 14):
    """The largest length L in [lo, hi) with f(L) == f(lo), f monotone."""
    v = f(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if f(mid) == v else (lo, mid)
    return lo


# ------------------------------------------------------------------ sparse probes
def probe(L, pos, fill, letter="C"):
    s = [fill] * L
    for p in pos:
        s[p - 1] = letter
    return "".join(s)


# (length, 1-based probe positions).  Single probes: K(x, y) = 1 + g^(i+j-2); the x rows 1, 63, 64, 65, 128, 129,
# 193 and Lx read column 0's powers in every strip (dn / g0col) and end in every owner lane; the y columns 1, 63,
# 64, 65, 128, 129 and Ly read the row-0 boundary.  Ly < 64 meets Lx > 64 (Lys = max(Ly, 64)).
X_SINGLE = [(1, (1,)), (63, (1,)), (63, (63,)), (64, (64,)), (65, (1,)), (65, (64,)), (65, (65,)), (128, (128,)),
            (129, (1,)), (129, (128,)), (129, (129,)), (193, (1,)), (193, (63,)), (193, (129,)), (193, (193,))]
Y_SINGLE = [(1, (1,)), (5, (1,)), (5, (5,)), (63, (63,)), (64, (64,)), (65, (1,)), (65, (65,)), (129, (63,)),
            (129, (128,)), (129, (129,)), (200, (1,)), (200, (64,)), (200, (129,)), (200, (200,))]
# two probes (p, p + 1 + run): a pair of them adds the chain (i, j) -> (i + 1 + e, j + 1 + d), a vertical run of e
# skipped rows and a horizontal run of d skipped columns; runs 0, 1, 62, 63, 64, 65, 127, 128 (and 20, for the 13-32
# bucket).  From row 1: rows 2 and 64 stay in strip 0, 65 crosses one strip boundary, 129 two; from row 60: 62 none,
# 125 and 126 one, 189 two.
RUNS = [(1, 0), (1, 62), (1, 63), (1, 127), (60, 1), (60, 64), (60, 65), (60, 128), (1, 20)]
X_DOUBLE = [(193, (p, p + 1 + r)) for p, r in RUNS]
Y_DOUBLE = [(200, (p, p + 1 + r)) for p, r in RUNS]
N_X = len(X_SINGLE) + len(X_DOUBLE)

# variant -> (x rows' fillers, x probe letter, y rows' fillers, x examples weighted, y examples weighted, naive)
# Against the y side's U and C the x side's A, G and R score 0 and its probe (C, or V = A/C/G with a third each)
# scores 1 with the probe C alone, so only probe-probe cells are non-zero in an x-y pair.
#   onehot   single sequences: the one-hot fast kernel
#   iupac    x filler R (A/G halves): the dyadic fast kernel (x-y, y-x, x-x; y-y stays one-hot)
#   aln2     x two rows (A.., G..), y two rows (U.., U..): columns hold counts (2, or 1 and 1), every pair dyadic
#   aln3     three rows: counts again (3, or 2 and 1), multiples of 1/256 as the packer tests them: the dyadic
#            kernel too (the sum s = 3 is exact, u / s rounds once: counted in F); not the general one
#   third    x probe V, a column of thirds: not dyadic, the general kernel
#   mixed    x weighted, y not: the general kernel under its no-weights rule (x-x and y-y one-hot)
#   naive    NaiveStringKernel: the general kernel's naive mode
VARIANTS = {
    "onehot": (("A",), "C", ("U",), None, None, False),
    "iupac": (("R",), "C", ("U",), None, None, False),
    "aln2": (("A", "G"), "C", ("U", "U"), None, None, False),
    "aln3": (("A", "A", "G"), "C", ("U", "U", "U"), None, None, False),
    "third": (("A",), "V", ("U",), None, None, False),
    "mixed": (("A",), "C", ("U",), True, False, False),
    "naive": (("A",), "C", ("U",), None, None, True),
}


def probe_bpp(L, pos):
    """Packed bpp of a probe example: each probe column p pairs with p + 4
    (p - 4 at the end) with probability 0.3, so its position weight is 0.7."""
    bpp = np.zeros(max(L * (L - 1) // 2, 1))
    for p in pos:
        q = p + 4 if p + 4 <= L else p - 4
        if q >= 1 and q not in pos:
            i, j = min(p, q) - 1, max(p, q) - 1
            bpp[i * L - i * (i + 1) // 2 + (j - i - 1)] = 0.3
    return bpp[: L * (L - 1) // 2] if L > 1 else bpp


def add_example(ds, om, rows, bpps, use_bp):
    ds.add("+1" if len(om) % 2 == 0 else "-1", rows, bpps if use_bp else None, th=0.01, use_bp=use_bp)
    om.append(po.OMData(rows, bpps if use_bp else None, 0.01, use_bp))


@functools.lru_cache(maxsize=None)
def probe_set(variant, use_bp):
    """(Dataset, [OMData], [first rows], [lengths], [has weights]) of a
    variant: examples 0 .. N_X - 1 the x side, the rest the y side."""
    xf, letter, yf, xw, yw, _ = VARIANTS[variant]
    ds, om, first, lens, hw = ska.Dataset(), [], [], [], []
    for side, fills, let, w in ((X_SINGLE + X_DOUBLE, xf, letter, xw), (Y_SINGLE + Y_DOUBLE, yf, "C", yw)):
        w = use_bp if w is None else w
        for L, pos in side:
            rows = [probe(L, pos, f, let) for f in fills]
            add_example(ds, om, rows, [probe_bpp(L, pos)] * len(rows), w)
            first.append(rows[0])
            lens.append(L)
            hw.append(w)
    return ds, om, first, lens, hw


def probe_positions():
    return [p for _, p in X_SINGLE + X_DOUBLE + Y_SINGLE + Y_DOUBLE]


def probe_kernel(variant, g):
    return ska.NaiveStringKernel(gap=g) if VARIANTS[variant][5] else ska.StringKernel(gap=g, match=1.0, mismatch=0.0)


def categories(ds, has_w):
    """Per ordered pair the kernel that takes it (0 one-hot, 1 dyadic, 2
    general), by the rules of pack_x.cpp / pairs_dag.cpp restated on the
    profiles the dataset holds."""
    oh, fast = [], []
    for k in range(len(ds)):
        c = ds.profile(k)[0][:, :4]
        oh.append(bool(np.all((np.sum(c == 1.0, axis=1) == 1) & (np.sum(c == 0.0, axis=1) == 3))))
        fast.append(bool(np.all(c * 256.0 == np.rint(c * 256.0)) and np.all(c.sum(axis=1) > 0.0)))
    n = len(ds)
    cat = np.full((n, n), 2)
    for a in range(n):
        for b in range(n):
            if has_w[a] == has_w[b]:
                cat[a, b] = 0 if oh[a] and oh[b] else (1 if fast[a] and fast[b] else 2)
    return cat


def expected_counts(cat, naive=False):
    """What Context.last_string() must report as pair counts for pairs of
    these categories."""
    c = [int(np.sum(cat == k)) for k in range(3)]
    return dict(onehot=0, dyadic=0, general=sum(c)) if naive else dict(onehot=c[0], dyadic=c[1], general=c[2])


def ran(ctx):
    """(pair counts, waves) of the last call."""
    ls = ctx.last_string()
    return {k: v[0] for k, v in ls.items()}, {k: v[1] for k, v in ls.items()}


def path_of(cat):
    return ("onehot", "dyadic", "general")[int(cat)]


def probe_tol(lens, cat, naive=False):
    """The tolerance matrix of a probe set: each pair at the F of the kernel
    that takes it."""
    n = len(lens)
    return np.array([[str_tol(lens[a], lens[b], "naive" if naive else path_of(cat[a, b])) for b in range(n)]
                     for a in range(n)])


def probe_reference(variant, use_bp, g):
    """K[x, y] over all ordered pairs of the set by the long-double twin."""
    _, om, first, _, _ = probe_set(variant, use_bp)
    n = len(om)
    if VARIANTS[variant][5]:
        return np.array([[po.naive_string_ld(first[a], first[b], g) for b in range(n)] for a in range(n)])
    return np.array([[po.si_str_ld(om[a], om[b], g, 1.0, 0.0) for b in range(n)] for a in range(n)])


THIRD = float(np.float32(1.0) / np.float32(3.0))   # the probe V against C: prof_subst = 1 * (1/3) * 1 / n, n = 1


def closed_form(g, naive=False, third=False):
    """[x single, y single] -> 1 + g^(i+j-2) (times g^2 in the naive mode,
    times THIRD for the probe letter V) with the double gap powers, and the
    transposed pairs likewise."""
    gp = gap_powers(g, 400)
    m = g * g if naive else (THIRD if third else 1.0)
    return np.array([[1.0 + m * gp[px[0] + py[0] - 2] for _, py in Y_SINGLE] for _, px in X_SINGLE])


def single_index():
    """Indices of the single-probe examples in a probe set: (x side, y side)."""
    return np.arange(len(X_SINGLE)), N_X + np.arange(len(Y_SINGLE))


# ------------------------------------------------------------------ dense sets
DENSE_CUTS = (("L120", 63), ("L120", 64), ("L120", 65), ("L200", 129), ("L300", 193))
ALN_LENGTHS = (40, 63, 64, 65, 120, 129, 193, 200, 300, 400)


@functools.lru_cache(maxsize=None)
def dense_sequences():
    """The sequences of stem_long_gaps' class sets (three each of L = 40 ..
    400) and five more cut from them to 63, 64, 65, 129 and 193."""
    seqs = [s for name in slg.CLASS_SETS for s in slg.class_set(name)]
    return tuple(seqs + [slg.class_set(name)[0][:L] for name, L in DENSE_CUTS])


def _of_length(L):
    return next(s for s in sorted(dense_sequences(), key=len) if len(s) >= L)[:L]


@functools.lru_cache(maxsize=None)
def dense_set(name):
    """(Dataset, [OMData], [lengths], [has weights]):
      single   the 23 sequences, folded (weighted): one-hot kernel
      dyadic   2- and 4-row alignments (alternating) of one sequence per
               length, unweighted, no gap columns: dyadic kernel
      aln3     3-row alignments likewise (count columns: dyadic kernel)
      general  the 3-row alignments with a B (C/G/U thirds) put into their
               first rows, one per 50 columns: general kernel
      mixed    single, the odd examples unweighted: weighted x unweighted
               pairs on the general kernel, the rest one-hot"""
    ds, om, lens, hw = ska.Dataset(), [], [], []
    if name in ("single", "mixed"):
        for k, s in enumerate(dense_sequences()):
            w = name == "single" or k % 2 == 0
            add_example(ds, om, [s], [ska.fold(s.lower())] if w else None, w)
            lens.append(len(s))
            hw.append(w)
        return ds, om, lens, hw
    for k, L in enumerate(ALN_LENGTHS):
        n_rows = 3 if name in ("aln3", "general") else (2 if k % 2 == 0 else 4)
        rows = mutate_alignment(_of_length(L), n_rows, 0x57E31 + L, gap=0.0)
        if name == "general":
            r0 = list(rows[0])
            r0[7::50] = "B" * len(r0[7::50])
            rows[0] = "".join(r0)
        add_example(ds, om, rows, None, False)
        lens.append(L)
        hw.append(False)
    return ds, om, lens, hw


DENSE_SETS = ("single", "dyadic", "aln3", "general", "mixed")
DENSE_KERNELS = ("su", "si")


def dense_kernel(which, g):
    return ska.StringKernel(gap=g, alpha=ALPHA) if which == "su" else \
        ska.StringKernel(gap=g, match=MATCH, mismatch=MISMATCH)


@functools.lru_cache(maxsize=None)
def dense_reference(name, which, g):
    _, om, _, _ = dense_set(name)
    f = (lambda a, b: po.su_str_ld(a, b, g, ALPHA)) if which == "su" else \
        (lambda a, b: po.si_str_ld(a, b, g, MATCH, MISMATCH))
    r = np.array([[f(a, b) for b in om] for a in om])
    r.setflags(write=False)
    return r


# ------------------------------------------------------------------ kinds 4, 5, 7
@functools.lru_cache(maxsize=None)
def sum_string_reference(name):
    """(k2, k3)[x, y]: the string parts of kinds 4 / 7 and 5 on a class set of
    stem_long_gaps (the kernels' default string parameters) by the twin."""
    _, om, _ = slg.built(name)
    p2, p3 = ska.SuStemStrKernel().params, ska.SiStemStrKernel().params
    k2 = np.array([[po.su_str_ld(a, b, p2.gap, p2.alpha) for b in om] for a in om])
    k3 = np.array([[po.si_str_ld(a, b, p3.gap, p3.match, p3.mismatch) for b in om] for a in om])
    for a in (k2, k3):
        a.setflags(write=False)
    return k2, k3


LOG_ULPS = 4   # kind 7: the two logs (1 ulp each as the device's log rounds), their products and the add


def sum_allowed(kind, stem, s, tol_stem, tol_str, p):
    """(expected, allowed absolute error) of kinds 4, 5 (stem + s) and 7
    (beta log stem + alpha log s): tol_stem stem + tol_str s for the sums of
    two non-negative parts; |beta| tol_stem + |alpha| tol_str plus LOG_ULPS
    ulps of each log term and of the result for kind 7."""
    if kind in (4, 5):
        exp = stem + s
        return exp, tol_stem * stem + tol_str * s + np.spacing(exp)
    a, b = p.beta * np.log(stem), p.alpha * np.log(s)
    exp = a + b
    return exp, abs(p.beta) * tol_stem + abs(p.alpha) * tol_str + LOG_ULPS * (
        np.spacing(np.abs(a)) + np.spacing(np.abs(b)) + np.spacing(np.abs(exp)))


# ------------------------------------------------------------------ visibility
# the buckets of tests/test_string_visibility_cpu.py: table -> index ranges zeroed one at a time
BUCKETS = [("C", 64, None), ("R", 64, None), ("wh", 13, 32), ("wh", 33, 64), ("wh", 65, None),
           ("wv", 13, 32), ("wv", 33, 64), ("wv", 65, None)]


def bucket_name(b):
    t, lo, hi = b
    return f"{t}[{lo}..{'' if hi is None else hi}]"


def masked_change(f_tab, g, lx, ly, bucket):
    """Relative change of K by the table twin f_tab(tables) when one bucket
    of the geometric tables is zeroed."""
    tab = po.string_tables(g, lx, ly)
    full = f_tab(tab)
    t, lo, hi = bucket
    tab[t][lo:(None if hi is None else hi + 1)] = 0
    return abs(f_tab(tab) - full) / full
