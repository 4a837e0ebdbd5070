"""The bound, the probes, the references and the tolerance of the 4-D stem
kernels' tests (tests/test_stem4d_probes.py, tests/test_stem4d_visibility_cpu.py,
tests/test_stem4d_oracle_twin.py and the full_dp / -b cases of
tests/test_stem4d.py).  DESIGN.md §7.3.

On a dense folded pair K is dominated by deep nestings with short loops
(K = 3.1e6 at L = 70, 1.8e14 at L = 130, gap 0.8): the leading 1, the shallow
terms and every long unpaired run are far below a 1e-6 comparison, and at
gap 0.8 a term with more than ~60 skipped positions is below it on any input
(0.8^62 < 1e-6).  The probes here are sparse -- a handful of dyadic base-pair
probabilities, zeros elsewhere, bp_bound 0 -- so that one chosen term is a
visible share of K, at gap 0.98 / 0.999 / 1.0 where a long run does not vanish.
Their reference is the closed form over the listed pairs in exact rationals;
the dense sets' reference is the long-double twin of the oracle's two DPs
(oracle/stem4d_generic.inc), live where it is cheap and from
tests/golden/stem4d_probes.npz (make_golden_4d_probes.py) above.
"""
import functools
import os
from fractions import Fraction
from typing import NamedTuple

import numpy as np

import stem_kernel_amd as ska
from oracle import pyoracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53
PROBE_CAP = 1e-11     # no probe's tolerance may exceed this
DENSE_CAP = 1e-8      # nor a dense case's this
SHARE = 1e-3          # every probe's targeted term is at least this share of K at its own gaps
BLIND = 1e-6          # the older tests' tolerance: what gap 0.8 hides (test_stem4d_visibility_cpu.py)
SEED = 0x4D57E3
DENSE_GAPS = (0.8, 0.98, 1.0)
DENSE_BANDS = (0, 1, 3, 8)


def f32(v) -> float:
    """An option as the kernel holds it (StemKernel4D rounds to float32, as the CLI parses)."""
    return float(np.float32(v))


# ------------------------------------------------------------------ the bound
def rounding_depth(n: int, m: int, banded: bool = False) -> int:
    """D_G (full_dp) or D_P (partial_dp): a bound on the roundings along any
    chain of double operations that carries one term into K0(0, n, 0, m) in
    the oracle's DP (oracle/sk_oracle.c stem4d_full, orc_stem4d_partial), the
    inputs (gap, stack, subst, the float probabilities) taken as given.

    Every value of the DP is a polynomial with non-negative coefficients in
    non-negative inputs -- partial_dp's boundary approximations only copy a
    neighbour's value or multiply it by g*g or a gap power -- so no sum
    cancels, and the double result is within D * 2^-53 (to first order) of
    the exact value, where D bounds the roundings any single term meets.

    One term of K is a stacking source at a cell (i, j, k, l) times a nesting
    path inside it (the G0 it reads), summed up to (0, n, 0, m):

    * G chains.  G0..G3 carry a term outward over j, i, l and k, one position
      per step, each step one product with g and one addition.  Along one
      nesting path i and k only grow and j and l only shrink, so all levels
      together take at most n + m steps: 2 (n + m) roundings.
    * Levels.  At each nesting level the term enters G3 (1 addition) and is
      handed G3 -> G2 -> G1 -> G0 (3 additions): 4 per level, at most
      floor(min(n, m) / 2) levels (each level uses two positions of both
      sequences): 2 min(n, m).
    * Base term.  The innermost g^((j-i)+(l-k)) is built by (j-i) + (l-k)
      products with g: at most n + m.  (Its positions are those the chains
      above do not cross, so this double counts; it is kept.)
    * Source.  g0 * stack * subst * bp_x * bp_y: 4 products.
    * K chain.  K3 -> K2 -> K1 -> K0 carry the source over k, l, i and j to
      (0, n, 0, m) by additions only, at most 2 (n + m) of them (the three
      hand-overs of the source's own cell included: a chain that hands over
      at a cell does not also step there).

      D_G = 5 (n + m) + 2 min(n, m) + 4

    partial_dp (banded) adds, per the reference's stem_kernel.cpp:113-280:

    * a second product with g where a chain step crosses the band's edge
      (G0 * g * g, G1 * g * g): at most one more per chain step, n + m;
    * the re-summation loop (:221-227) and the K3 / G3 reads off the band
      (:233-235) multiply by gpw[l - k] (l - k <= m roundings in the table,
      one product) after up to m additions: 2 m + 1.  In the reference these
      read K3 / G3 of diagonal cells (ll, ll), which no statement writes
      (every update has k <= l - 1), so they add exact zeros; the count is
      kept once for a kernel that forms these boundary values otherwise.

      D_P = D_G + (n + m) + 2 m + 1
    """
    d = 5 * (n + m) + 2 * min(n, m) + 4
    return d + (n + m) + 2 * m + 1 if banded else d


def pair_count(seq: str, bpp, model=0, bound=0.0, loop=3) -> int:
    """The pairs (a, b), a < b, of one sequence that a stacking source can
    use: BPMat::prob(a, b) > bp_bound, as the oracle's bp4_prob forms it."""
    L = len(seq)
    if L < 2:
        return 0
    if model == 0:
        return int(np.count_nonzero(np.asarray(bpp).astype(np.float32) > np.float32(bound)))
    c = np.frombuffer(seq.lower().encode(), np.uint8)
    a, b = c[:, None], c[None, :]
    ok = ((a == ord("a")) & (b == ord("u"))) | ((a == ord("u")) & (b == ord("a"))) | \
         ((a == ord("g")) & (b == ord("c"))) | ((a == ord("c")) & (b == ord("g")))
    if model == 2:
        ok |= ((a == ord("g")) & (b == ord("u"))) | ((a == ord("u")) & (b == ord("g")))
    i, j = np.arange(L)[:, None], np.arange(L)[None, :]
    return int(np.count_nonzero(ok & (i + 1 + loop <= j))) if np.float32(1.0) > np.float32(bound) else 0


def tol(n: int, m: int, sx: int, sy: int, banded: bool = False) -> float:
    """Relative tolerance of a GPU value against the long-double twin or the
    closed form: 4 (D + S) 2^-53.  S = sx * sy, the pair's non-zero stacking
    sources (sx, sy: pair_count of x and of y): the K-sum kernels add the
    sources per lane, per wave and per i instead of along the K chain, and no
    order of summing S non-negative terms makes more than S additions -- D + S
    holds for any schedule.  The factor 4 (as in stem_long_gaps.stem_tol)
    covers the kernels' factorings -- gap-power tables, pre-combined spans,
    closed forms of the base terms -- which distribute and reassociate the
    same non-negative terms, and the reference's own rounding."""
    return 4.0 * (rounding_depth(n, m, banded) + sx * sy) * U


# ------------------------------------------------------------------ the sparse probes
class Probe(NamedTuple):
    name: str
    family: str     # table_end, nested, seam, long_x
    group: str      # the probes of one group share a pairs() call: one y length class each
    x: str
    xp: tuple       # ((a, b, p), ...): 0-based a < b with bp(a, b) = p, zeros elsewhere
    y: str
    yp: tuple
    target: tuple   # ("x" | "y", (a, b)): the inner pair whose terms the probe isolates; () for table_end
    run: int        # the longest run of skipped positions the targeted term crosses


def _seq(L, k, ends):
    """A random sequence of length L with the given residues at the pairs' ends."""
    s = list(ska.random_sequences(1, L, SEED + k)[0])
    for pos, ch in ends.items():
        s[pos] = ch
    return "".join(s)


OUT, INN = ("G", "C"), ("A", "U")   # end bases of the outer and of the inner pairs


def _two(L, k, outer, inner, p=(0.75, 0.5), bases=(OUT, INN)):
    ends = {}
    for (a, b), (ca, cb) in zip((outer, inner), bases):
        ends[a], ends[b] = ca, cb
    return _seq(L, k, ends), ((outer[0], outer[1], p[0]), (inner[0], inner[1], p[1]))


def _one(L, k, p):
    return _seq(L, k, {0: "G", L - 1: "C"}), ((0, L - 1, p),)


TABLE_END_M = (62, 63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024, 1100)   # against n = 12
TABLE_END_N = (2047, 2048, 2049)                                            # against m = 40
RUNS = (0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)
NESTED_M = (140, 100, 60)   # y length classes of the k / l side sweeps: CPL 4, 2, 1 (W = 8 each)
NESTED_SHORT_Y = 8          # the y of the i / j side sweeps: W = 8 - 3 = 5


def _table_end(scale=None):
    out = []
    for m in TABLE_END_M:
        if scale and m > scale:
            continue
        x, xp = _one(12, 1, 0.75)
        y, yp = _one(m, 100 + m, 0.75)
        out.append(Probe(f"te_m{m}", "table_end", f"m{m}", x, xp, y, yp, (), (12 - 2) + (m - 2)))
    for n in TABLE_END_N if not scale else (scale - 1, scale):
        x, xp = _one(n, 200 + n, 0.75)
        y, yp = _one(40, 2, 0.75)
        out.append(Probe(f"te_n{n}", "table_end", f"n{n}", x, xp, y, yp, (), (n - 2) + (40 - 2)))
    # the G3 source does not fire: the term carries subst
    x, xp = _one(12, 1, 0.75)
    y, yp = _one(128, 100 + 128, 0.75)
    y = "A" + y[1:]
    out.append(Probe("te_m128_subst", "table_end", "m128s", x, xp, y, yp, (), 10 + 126))
    return out


def _nested(scale=None):
    """Outer and inner pair adjacent in the short sequence; in the long one the
    inner pair sits r positions inside the outer on one side (k, l: the run
    is in y; i, j: x and y exchanged, the run is in x) and next to it on the
    other."""
    out = []
    short, sp = _two(12, 3, (0, 11), (1, 10))
    for m in NESTED_M:
        for side in "kl":
            for r in RUNS:
                if 1 + r >= m - 2 - 8:   # keep an inner loop of 8 or more
                    continue
                inner = (1 + r, m - 2) if side == "k" else (1, m - 2 - r)
                y, yp = _two(m, 1000 * m + r, (0, m - 1), inner)
                out.append(Probe(f"ne_{side}{r}_m{m}", "nested", f"m{m}", short, sp, y, yp, ("y", inner), r))
    tiny, tp = _two(NESTED_SHORT_Y, 4, (0, NESTED_SHORT_Y - 1), (1, NESTED_SHORT_Y - 2))
    n = 140
    for side in "ij":
        for r in RUNS:
            inner = (1 + r, n - 2) if side == "i" else (1, n - 2 - r)
            x, xp = _two(n, 7000 + (r if side == "i" else 500 + r), (0, n - 1), inner)
            out.append(Probe(f"ne_{side}{r}_y{NESTED_SHORT_Y}", "nested", f"y{NESTED_SHORT_Y}", x, xp, tiny, tp,
                             ("x", inner), r))
    # the G3 source does not fire: on the inner pair (the nested term vanishes,
    # the inner sources carry subst) and on the outer pair (its source carries subst)
    for r in (8, 64):
        y, yp = _two(140, 9000 + r, (0, 139), (1 + r, 138), bases=(OUT, ("C", "U")))
        out.append(Probe(f"ne_k{r}_m140_inner_subst", "nested", "m140", short, sp, y, yp, ("y", (1 + r, 138)), r))
        y, yp = _two(140, 9100 + r, (0, 139), (1 + r, 138), bases=(("G", "A"), INN))
        out.append(Probe(f"ne_k{r}_m140_outer_subst", "nested", "m140", short, sp, y, yp, ("y", (1 + r, 138)), r))
    return out


def _seam(m=1100, seams=(512, 1024), run=(30, 1000)):
    """Long y (k tiles of 512): the outer y pair's k just left of a tile seam
    and the inner's just right, the same on the l side, and one run (outer k,
    skipped positions) = (30, 1,000) across both seams: the outer pair's k
    lies in the first tile and the inner's in the third, so the nested term's
    G3 chain passes through the whole middle tile and both boundary-column
    hand-overs."""
    out = []
    short, sp = _two(12, 5, (0, 11), (1, 10))
    s0, s1 = seams
    for a, b in ((s0 - 1, s0), (s0 - 2, s0 + 1), (s1 - 1, s1)):
        y, yp = _two(m, 20000 + a, (a, m - 1), (b, m - 2))
        out.append(Probe(f"se_k{a}_{b}", "seam", "seam", short, sp, y, yp, ("y", (b, m - 2)), b - a - 1))
        y, yp = _two(m, 21000 + a, (0, b), (1, a))
        out.append(Probe(f"se_l{a}_{b}", "seam", "seam", short, sp, y, yp, ("y", (1, a)), b - a - 1))
    o, r = run
    inner = (o + 1 + r, m - 2)
    assert o < s0 and s1 <= inner[0] < inner[1] - 4, (o, inner, seams)   # first tile | third tile, a loop inside
    y, yp = _two(m, 22000, (o, m - 1), inner)
    out.append(Probe(f"se_run{r}", "seam", "seam", short, sp, y, yp, ("y", inner), r))
    return out


def _long_x(sizes=((700, 600), (2100, 2000))):
    """Long x against m = 40: runs on the i and on the j side (n = 700: the
    column kernel with x in LDS, many groups and rounds; n = 2,100: past its
    x limit, the span kernel)."""
    out = []
    y, yp = _two(40, 6, (0, 39), (1, 38))
    for n, r in sizes:
        for side in "ij":
            inner = (1 + r, n - 2) if side == "i" else (1, n - 2 - r)
            x, xp = _two(n, 30000 + n + (side == "j"), (0, n - 1), inner)
            out.append(Probe(f"lx_{side}{r}_n{n}", "long_x", f"n{n}", x, xp, y, yp, ("x", inner), r))
    return out


FAMILIES = ("table_end", "nested", "seam", "long_x")


@functools.lru_cache(maxsize=None)
def probes(family, small=False):
    """The probes of a family; small: the family scaled down to sequences of
    at most 140 (the twin's cost), with the same construction."""
    if family == "table_end":
        return tuple(_table_end(128 if small else None))
    if family == "nested":
        return tuple(_nested())
    if family == "seam":
        return tuple(_seam(140, (64, 128), (10, 120)) if small else _seam())
    if family == "long_x":
        return tuple(_long_x(((140, 100), (120, 90))) if small else _long_x())
    raise KeyError(family)


def groups(family, small=False):
    """{group: [Probe]} in order of first appearance."""
    out = {}
    for pr in probes(family, small):
        out.setdefault(pr.group, []).append(pr)
    return out


def probe_gaps(pr):
    """The gaps a probe runs at, where its targeted term is visible: 0.98
    for sequences up to 140 (the term skips at most ~150 positions, loops
    included), 0.999 above, and the boundary 1.0 -- as the kernel holds
    them."""
    return (f32(0.98), 1.0) if max(len(pr.x), len(pr.y)) <= 140 else (f32(0.999), 1.0)


DEFAULT_GAP = f32(0.8)   # every family runs once here too: it guards the leading 1 and the local terms


def packed_bpp(L, pairs):
    """Strict upper triangle, row-major (the Dataset's and the oracle's layout)."""
    b = np.zeros(L * (L - 1) // 2)
    for a, c, p in pairs:
        assert 0 <= a < c < L
        b[a * L - a * (a + 1) // 2 + (c - a - 1)] = p
    return b


def closed_form(pr, gap, stack=1.0, subst=0.5, drop=None, nested_only=False) -> Fraction:
    """K of a probe in exact rationals of the double parameters.  With
    half-open planes [i, j) x [k, l) as in the oracle,

      G0(i,j,k,l) = g^((j-i)+(l-k))
                    + sum g^((a-i)+(j-b)+(c-k)+(l-d)) G0(a+1, b-1, c+1, d-1)

    over the x pairs [a, b) within [i, j) and the y pairs [c, d) within
    [k, l) whose end bases are equal (x[a] == y[c] and x[b-1] == y[d-1]: the
    G3 source), and

      K = 1 + sum stack (1 | subst) bp_x bp_y G0(a+1, b-1, c+1, d-1)

    over every x pair times every y pair (1 where the end bases are equal).
    drop = ("x" | "y", (a, b)): without that pair; nested_only: the pair
    keeps its own sources and is dropped from the G0 sums alone, which
    removes exactly the terms that reach it through an enclosing pair's
    chains (the terms that carry g^run)."""
    g, st, su = Fraction(gap), Fraction(stack), Fraction(subst)
    x, y = pr.x.lower(), pr.y.lower()
    gone = lambda w, a, b: drop == (w, (a, b))
    xn = [(a, b + 1, Fraction(p)) for a, b, p in pr.xp if not gone("x", a, b)]
    yn = [(c, d + 1, Fraction(p)) for c, d, p in pr.yp if not gone("y", c, d)]
    xp = [(a, b + 1, Fraction(p)) for a, b, p in pr.xp] if nested_only else xn
    yp = [(c, d + 1, Fraction(p)) for c, d, p in pr.yp] if nested_only else yn
    same = lambda a, b, c, d: x[a] == y[c] and x[b - 1] == y[d - 1]

    @functools.lru_cache(maxsize=None)
    def g0(i, j, k, l):
        v = g ** ((j - i) + (l - k))
        for a, b, _ in xn:
            if i <= a and b <= j:
                for c, d, _ in yn:
                    if k <= c and d <= l and same(a, b, c, d):
                        v += g ** ((a - i) + (j - b) + (c - k) + (l - d)) * g0(a + 1, b - 1, c + 1, d - 1)
        return v

    K = Fraction(1)
    for a, b, p in xp:
        for c, d, q in yp:
            K += st * (1 if same(a, b, c, d) else su) * p * q * g0(a + 1, b - 1, c + 1, d - 1)
    return K


@functools.lru_cache(maxsize=None)
def probe_ref(name_key, gap, stack=1.0, subst=0.5) -> float:
    """closed_form rounded once, cached per (family, small, name)."""
    family, small, name = name_key
    pr = next(p for p in probes(family, small) if p.name == name)
    return float(closed_form(pr, gap, stack, subst))


def probe_tol(pr, banded=False) -> float:
    return tol(len(pr.x), len(pr.y), len(pr.xp), len(pr.yp), banded)


def share(pr, gap, stack=1.0, subst=0.5, nested_only=False) -> float:
    """The relative change of K when the probe's targeted pair is removed
    (nested_only: from the G0 sums alone, the terms that cross the run); for
    a table-end probe (K - 1) / K."""
    K = closed_form(pr, gap, stack, subst)
    if not pr.target:
        return float((K - 1) / K)
    return float(abs(K - closed_form(pr, gap, stack, subst, pr.target, nested_only)) / K)


def exchanged(pr):
    """The probe with x and y exchanged (K is symmetric in them)."""
    t = ({"x": "y", "y": "x"}[pr.target[0]], pr.target[1]) if pr.target else ()
    return pr._replace(x=pr.y, xp=pr.yp, y=pr.x, yp=pr.xp, target=t)


def probe_dataset(prs):
    """(Dataset, x indices, y indices) of a group's probes: every distinct
    (sequence, pairs) once."""
    items, xi, yi = {}, [], []
    for pr in prs:
        for s, pp, idx in ((pr.x, pr.xp, xi), (pr.y, pr.yp, yi)):
            idx.append(items.setdefault((s, pp), len(items)))
    seqs = [s for s, _ in items]
    ds = ska.Dataset.from_sequences(seqs, bpp=[packed_bpp(len(s), pp) for s, pp in items])
    return ds, np.array(xi, np.int32), np.array(yi, np.int32)


def twin_of_probe(pr, gap, stack=1.0, subst=0.5, band=0, cut=-1) -> float:
    return po.stem4d_ld(pr.x.lower(), packed_bpp(len(pr.x), pr.xp), pr.y.lower(), packed_bpp(len(pr.y), pr.yp),
                        gap, stack, subst, 0.0, 0, 3, band, cut)


# ------------------------------------------------------------------ the dense sets
def suite_seqs():
    """The sequences of tests/test_stem4d.py's Grams."""
    s = ska.random_sequences(4, 30, 0x5EED0003) + ska.random_sequences(2, 70, 0x5EED0013)
    s += ska.random_sequences(1, 64, 3) + ska.random_sequences(1, 63, 4)
    s += ["GGGGAAAACCCC", "A", "ACGUN"]
    return s


def l130():
    return ska.random_sequences(2, 130, 0x5EED0043)


@functools.lru_cache(maxsize=None)
def dense_set(name):
    """(sequences, [(x, y)]): `suite` the Gram of suite_seqs(); `col` the Gram
    of test_stem4d.py's column-kernel set (gap 0.8, full_dp only); `l130` the
    two L = 130 sequences; `lop` the lopsided 24 x 300 / 457 pairs, where
    long runs reach the compared digits."""
    if name in ("suite", "col", "l130"):
        seqs = {"suite": suite_seqs(), "col": suite_seqs() + ["", "G"] + l130(), "l130": l130()}[name]
        return tuple(seqs), tuple((int(a), int(b)) for a, b in zip(*np.triu_indices(len(seqs))))
    if name == "lop":
        xs = ska.random_sequences(2, 24, 0x5EED0061) + ["GGGCGCAAGCCU"]
        ys = ska.random_sequences(1, 300, 0x5EED0062) + ska.random_sequences(1, 457, 0x5EED0063)
        return tuple(xs + ys), ((0, 3), (1, 3), (2, 4), (0, 4), (2, 3))
    if name == "tiled":
        return tuple(ska.random_sequences(1, 24, 0x5EED0081) + ska.random_sequences(1, 1040, 0x5EED0082)), ((0, 1),)
    raise KeyError(name)


DENSE_SETS = ("suite", "l130", "lop")
TILED_BAND = 100   # the banded pair over k tiles: 24 x 1,040, its windows hold k = 512 for four values of i


@functools.lru_cache(maxsize=None)
def folded(seq):
    b = ska.fold(seq.lower()) if seq else np.zeros(0)
    b.setflags(write=False)
    return b


def twin(xa, xb, p, cut=-1) -> float:
    """The long-double twin at a kernel's parameters (full_dp or -b)."""
    m0 = p.bp_model == 0
    return po.stem4d_ld(xa.lower(), folded(xa) if m0 else None, xb.lower(), folded(xb) if m0 else None, p.gap,
                        p.stack, p.subst, p.bp_bound, p.bp_model, p.loop, p.len_band, cut)


def _pkey(p):
    return (p.gap, p.stack, p.subst, p.bp_bound, p.bp_model, p.loop, p.len_band)


@functools.lru_cache(maxsize=None)
def _twin_cached(xa, xb, key):
    class P:
        gap, stack, subst, bp_bound, bp_model, loop, len_band = key
    return twin(xa, xb, P)


def twin_values(seqs, pairs, p) -> np.ndarray:
    """Live twin values of (seqs[a], seqs[b]) for the pairs, computed once per
    (pair, parameters) and shared among the tests."""
    assert p.ali_bound == 0.0
    return np.array([_twin_cached(seqs[a], seqs[b], _pkey(p)) for a, b in pairs])


def pair_tols(seqs, pairs, p) -> np.ndarray:
    """tol() of every pair at a kernel's parameters."""
    cnt = {s: pair_count(s, folded(s) if p.bp_model == 0 else None, p.bp_model, p.bp_bound, p.loop)
           for s in set(seqs)}
    return np.array([tol(len(seqs[a]), len(seqs[b]), cnt[seqs[a]], cnt[seqs[b]], p.len_band > 0)
                     for a, b in pairs])


def dense_key(name, gap, band):
    return f"{name}_g{gap}_b{band}"


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "stem4d_probes.npz"))


def dense_ref(name, gap, band) -> np.ndarray:
    """Twin values of a dense set's pairs from the golden file (gap: the
    nominal 0.8 / 0.98 / 1.0; the values are at the float32 gap)."""
    r = golden()[dense_key(name, gap, band)]
    r.setflags(write=False)
    return r


def excess(got, ref, tols):
    """(max error / tolerance, max relative error, largest tolerance)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rel = np.abs(got - ref) / np.abs(ref)
    return float(np.max(rel / tols)), float(np.max(rel)), float(np.max(tols))
