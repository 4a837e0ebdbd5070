"""The profile string kernels (profile_string.hip: one-hot fast, dyadic fast,
general, naive mode) where boundary gaps, long runs, launch shapes and
two-set calls reach the compared digits.  Every value is compared with the
long-double twin of the oracle's DP (oracle/sk_oracle.c: _ld) at the
tolerance 4 D 2^-53 of tests/string_long_gaps.py (D: the pair's rounding
depth; at most 1e-11 on every fixture), every reference value is finite,
no pair is left out, and every call asserts the kernels that took its pairs
and their waves per workgroup through Context.last_string().
tests/test_string_visibility_cpu.py zeroes the column-0 powers, the row-0
boundary and the run weights by length at each case's own parameters and
says which cases move by 100 tolerances or more.  DESIGN.md §7.2.

  a. sparse probes, gap 0.98 / 0.999 / 1: one or two non-zero cells, so K - 1
     is g^(i+j-2) (and one chain over a vertical and a horizontal run); the
     unweighted ones also against that closed form;
  b. dense class sets, gap 0.8 / 0.98 / 1, both score tables, L = 40 .. 400
     with 63, 64, 65, 129, 193: singles, 2- / 4-row, 3-row, third-column and
     weighted x unweighted sets;
  c. kinds 4, 5 and 7 on the class sets of tests/stem_long_gaps.py at every
     L: stem part from tests/golden/stem_long_gaps.npz, string part live;
  d. launch shapes: y lengths on either side of 4 -> 2 -> 1 waves of the
     general kernel, of 4 -> 3 waves of either fast kernel, of the fast ->
     general hand-over, and one past the LDS limit (an error);
  e. two sets (test_matrix and test_row in both orders; sk_pairs takes one
     set): the x set longer than every y and the reverse (the gap-power
     table's length, the fast paths' second-set table offsets), one-hot,
     dyadic, and one call with pairs of all three categories.

Measured GPU error per family: see MEASURED below (pytest -s prints them).
"""
import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem_long_gaps as slg
from tests import string_long_gaps as sg

pytestmark = pytest.mark.gpu

# From a run on an MI355X: family -> (max relative error, max error / tolerance).
MEASURED = {
    "sparse probes, one-hot / dyadic (iupac, aln2, aln3) kernels": (1.7e-14, 8.0e-3),
    "sparse probes, general kernel (third, mixed) and naive mode": (2.4e-15, 9.0e-3),
    "dense sets, one-hot / dyadic / general kernels": (5.2e-15, 2.2e-3),
    "kinds 4 and 5 (error / allowed)": (None, 1.6e-3),
    "kind 7 (absolute error, error / allowed)": (7.1e-15, 5.5e-3),
    "launch shapes": (2.2e-16, 1.6e-4),
    "two sets": (2.2e-16, 5.2e-5),
}


def _all_pairs(n):
    x, y = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    return x, y


def _check(what, got, ref, tol):
    assert np.all(np.isfinite(ref)), what
    err = np.abs(np.asarray(got) - ref)
    rel, worst = float(np.max(err / ref)), float(np.max(err / (tol * ref)))
    print(f"{what}: max rel err {rel:.3g}, err / tolerance {worst:.3g}, tolerance up to {np.max(tol):.3g}")
    assert np.max(tol) <= sg.TOL_CAP, what
    assert worst <= 1.0, (what, worst)


# ------------------------------------------------------------------ a. sparse probes
PROBE_CASES = [(v, bp) for v in sg.VARIANTS for bp in (False, True) if not (v == "mixed" and not bp)]


def _probe_counts(variant, n):
    nx, ny = sg.N_X, n - sg.N_X
    return {"onehot": dict(onehot=n * n, dyadic=0, general=0),
            # (the x example of length 1 is the probe letter alone: one-hot)
            "iupac": dict(onehot=(ny + 1) ** 2, dyadic=n * n - (ny + 1) ** 2, general=0),
            "aln2": dict(onehot=0, dyadic=n * n, general=0),   # the y side's columns hold the count 2, not 1
            "aln3": dict(onehot=0, dyadic=n * n, general=0),
            "third": dict(onehot=ny * ny, dyadic=0, general=n * n - ny * ny),
            "mixed": dict(onehot=nx * nx + ny * ny, dyadic=0, general=2 * nx * ny),
            "naive": dict(onehot=0, dyadic=0, general=n * n)}[variant]


@pytest.mark.parametrize("g", sg.GAPS)
@pytest.mark.parametrize("variant,use_bp", PROBE_CASES)
def test_sparse_probes(gpu_ctx, variant, use_bp, g):
    ds, om, first, lens, hw = sg.probe_set(variant, use_bp)
    naive = sg.VARIANTS[variant][5]
    n = len(ds)
    cat = sg.categories(ds, hw)
    tol = sg.probe_tol(lens, cat, naive)
    ref = sg.probe_reference(variant, use_bp, g)
    x, y = _all_pairs(n)
    got = gpu_ctx.pairs(ds, sg.probe_kernel(variant, g), x, y).reshape(n, n)
    counts, waves = sg.ran(gpu_ctx)
    assert counts == sg.expected_counts(cat, naive) == _probe_counts(variant, n), counts
    assert all(waves[k] == (4 if counts[k] else 0) for k in counts), waves
    _check(f"probes {variant} use_bp {use_bp} gap {g}", got, ref, tol)
    # the x side against the y side, both orders: only probe cells score
    xs, ys = np.arange(sg.N_X), np.arange(sg.N_X, n)
    for a, b in ((xs, ys), (ys, xs)):
        blk = np.ix_(a, b)
        assert np.all(ref[blk] - 1.0 >= 100.0 * tol[blk] * ref[blk]), (variant, "a probe cell is empty")
    # single probes whose pair runs without weights: 1 + g^(i+j-2)
    sx, sy = sg.single_index()
    if not (hw[sx[0]] and hw[sy[0]]) or naive:
        cf = sg.closed_form(g, naive, third=variant == "third")
        for what, blk, c in (("x-y", np.ix_(sx, sy), cf), ("y-x", np.ix_(sy, sx), cf.T)):
            assert np.all(np.abs(ref[blk] - c) <= tol[blk] * c), (variant, what, "twin against the closed form")
            assert np.all(np.abs(got[blk] - c) <= tol[blk] * c), (variant, what, "GPU against the closed form")


# ------------------------------------------------------------------ b. dense class sets
@pytest.mark.parametrize("g", sg.DENSE_GAPS)
@pytest.mark.parametrize("which", sg.DENSE_KERNELS)
@pytest.mark.parametrize("name", sg.DENSE_SETS)
def test_dense_sets(gpu_ctx, name, which, g):
    ds, om, lens, hw = sg.dense_set(name)
    n = len(ds)
    cat = sg.categories(ds, hw)
    tol = sg.probe_tol(lens, cat)
    ref = sg.dense_reference(name, which, g)
    x, y = _all_pairs(n)
    got = gpu_ctx.pairs(ds, sg.dense_kernel(which, g), x, y).reshape(n, n)
    counts, waves = sg.ran(gpu_ctx)
    nw, nu = sum(hw), n - sum(hw)
    want = {"single": dict(onehot=n * n, dyadic=0, general=0), "dyadic": dict(onehot=0, dyadic=n * n, general=0),
            "aln3": dict(onehot=0, dyadic=n * n, general=0), "general": dict(onehot=0, dyadic=0, general=n * n),
            "mixed": dict(onehot=nw * nw + nu * nu, dyadic=0, general=2 * nw * nu)}[name]
    assert counts == sg.expected_counts(cat) == want, counts
    assert all(waves[k] == (4 if counts[k] else 0) for k in counts), waves
    _check(f"dense {name} {which} gap {g} (K up to {ref.max():.3g})", got, ref, tol)


# ------------------------------------------------------------------ c. kinds 4, 5 and 7
@pytest.mark.parametrize("g,band", sg.SUM_PARAMS)
@pytest.mark.parametrize("name", list(slg.CLASS_SETS))
def test_sum_kinds(gpu_ctx, name, g, band):
    ds, om, st = slg.built(name)
    n = len(ds)
    lens = [po.oracle().orc_mdata_seq_len(o.h) for o in om]
    tol_stem, tol_str = slg.tol_matrix(st), sg.tol_matrix(lens, path="onehot")
    assert tol_stem.max() <= slg.TOL_CAP and tol_str.max() <= sg.TOL_CAP
    ref = slg.reference(name, g, band)
    k2, k3 = sg.sum_string_reference(name)
    x, y = _all_pairs(n)
    for kind in (4, 5, 7):
        kern = slg.kernel(kind, g, band)
        stem, s = (ref["si"], k3) if kind == 5 else (ref["su"], k2)
        assert np.all(np.isfinite(s)) and np.all(stem > 0)
        exp, allowed = sg.sum_allowed(kind, stem, s, tol_stem, tol_str, kern.params)
        got = gpu_ctx.pairs(ds, kern, x, y).reshape(n, n)
        counts, waves = sg.ran(gpu_ctx)
        assert counts == dict(onehot=n * n, dyadic=0, general=0) and waves["onehot"] == 4, (counts, waves)
        err = np.abs(got - exp)
        print(f"{name} loop_gap {g} band {band} kind {kind}: max |err| {err.max():.3g}, err / allowed "
              f"{np.max(err / allowed):.3g}, stem / str {np.min(stem / s):.3g} .. {np.max(stem / s):.3g}")
        assert np.all(err <= allowed), (name, g, band, kind)


# ------------------------------------------------------------------ d. launch shapes
def _shape_cases():
    """(path, y length, kernel that must run, its waves): the y lengths on
    either side of every change of launch shape, from the LDS model."""
    g4 = sg.last_below(sg.general_waves)
    g2 = sg.last_below(sg.general_waves, g4 + 1)
    g1 = sg.last_below(sg.general_waves, g2 + 1)
    d4 = sg.last_below(lambda L: sg.fast_waves(L, False))
    o4 = sg.last_below(lambda L: sg.fast_waves(L, True))
    h = sg.last_below(lambda L: sg.fast_waves(L, False) > 0)
    cases = [("general", L) for L in (g4, g4 + 1, g2, g2 + 1, g1)]
    cases += [("dyadic", L) for L in (d4, d4 + 1, h, h + 1)] + [("onehot", L) for L in (o4, o4 + 1, h, h + 1)]
    out = []
    for path, L in cases:
        fw = sg.fast_waves(L, path == "onehot")
        kern, w = (path, fw) if path != "general" and fw else ("general", sg.general_waves(L))
        out.append((path, L, kern, w))
    assert [c[3] for c in out[:5]] == [4, 2, 2, 1, 1] and out[5][3] == 4 and out[6][3] < 4 and out[9][3] == 4 \
        and out[10][3] < 4 and out[7][2] == "dyadic" and out[8][2] == "general" and out[11][2] == "onehot" \
        and out[12][2] == "general" and sg.general_waves(g1 + 1) == 0
    return out, g1


SHAPE_CASES, LDS_LIMIT = _shape_cases()
X_SHAPE = [(65, (1,)), (65, (64,)), (65, (65,))]


def _shape_set(path, ly):
    """Three short x examples and four y examples of length ly with the
    probe in the first column, the last, and on either side of an interior
    strip boundary; unweighted."""
    fill, letter = ("R", "C") if path == "dyadic" else (("A", "V") if path == "general" else ("A", "C"))
    jb = 64 * max(1, ly // 128)
    ypos = [(1,), (ly,), (jb,), (jb + 1,)]
    ds, om = ska.Dataset(), []
    for L, pos in X_SHAPE:
        sg.add_example(ds, om, [sg.probe(L, pos, fill, letter)], None, False)
    for pos in ypos:
        sg.add_example(ds, om, [sg.probe(ly, pos, "U")], None, False)
    return ds, om, [p for _, p in X_SHAPE] + ypos


@pytest.mark.parametrize("path,ly,kern,w", SHAPE_CASES)
def test_launch_shapes(gpu_ctx, path, ly, kern, w):
    ds, om, pos = _shape_set(path, ly)
    g = 0.999
    gp = sg.gap_powers(g, 2 * ly + 2)
    nx = len(X_SHAPE)
    x, y = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(nx), np.arange(nx, len(ds)), indexing="ij"))
    tol = sg.str_tol(65, ly, kern)
    for what, a, b in (("short x, long y", x, y), ("long x, short y", y, x)):
        got = gpu_ctx.pairs(ds, ska.StringKernel(gap=g, match=1.0, mismatch=0.0), a, b)
        counts, waves = sg.ran(gpu_ctx)
        assert counts == {k: (len(a) if k == kern else 0) for k in counts}, (counts, kern)
        assert waves == {k: (w if k == kern else 0) for k in waves}, (waves, kern, w)
        ref = np.array([po.si_str_ld(om[i], om[j], g, 1.0, 0.0) for i, j in zip(a, b)])
        cf = np.array([1.0 + (sg.THIRD if path == "general" else 1.0) * gp[pos[i][0] + pos[j][0] - 2]
                       for i, j in zip(a, b)])
        _check(f"launch shape {path} y length {ly} ({kern}, {w} waves), {what}", got, ref, tol)
        assert np.all(np.abs(got - cf) <= tol * cf) and np.all(ref - 1.0 >= 100 * tol)


@pytest.mark.parametrize("path", ["general", "onehot"])
def test_past_the_lds_limit(gpu_ctx, path):
    ds, _, _ = _shape_set(path, LDS_LIMIT + 1)
    with pytest.raises(ska.StemKernelError, match="sequence too long for string kernel LDS"):
        gpu_ctx.pairs(ds, ska.StringKernel(gap=0.999, match=1.0, mismatch=0.0), [0], [len(X_SHAPE)])


# ------------------------------------------------------------------ e. two sets
LONG_X = [(500, (1,)), (500, (449,)), (500, (500,))]
SHORT_Y = [(200, (1,)), (200, (200,)), (65, (65,)), (5, (5,))]


def _two_sets(kind):
    """A: three x-side examples of length 500, longer than every example of
    B, four y-side examples; kind onehot / dyadic (filler R) / all3 (one
    one-hot, one dyadic, one with a third-column probe)."""
    styles = {"onehot": [("A", "C")] * 3, "dyadic": [("R", "C")] * 3, "all3": [("A", "C"), ("R", "C"), ("A", "V")]}[kind]
    A, oa, B, ob = ska.Dataset(), [], ska.Dataset(), []
    for (L, pos), (fill, letter) in zip(LONG_X, styles):
        sg.add_example(A, oa, [sg.probe(L, pos, fill, letter)], None, False)
    for L, pos in SHORT_Y:
        sg.add_example(B, ob, [sg.probe(L, pos, "U")], None, False)
    return A, oa, B, ob


@pytest.mark.parametrize("g", [0.98, 1.0])
@pytest.mark.parametrize("kind", ["onehot", "dyadic", "all3"])
def test_two_sets(gpu_ctx, kind, g):
    A, oa, B, ob = _two_sets(kind)
    kern = ska.StringKernel(gap=g, match=1.0, mismatch=0.0)
    gp = sg.gap_powers(g, 1100)
    na, nb = len(A), len(B)
    per = {"onehot": dict(onehot=1, dyadic=0, general=0), "dyadic": dict(onehot=0, dyadic=1, general=0),
           "all3": None}[kind]

    def want(n_a, n_b):  # pairs of n_a examples of A with n_b of B, per kernel
        if per is None:
            assert n_a in (1, na)
            return None if n_a == 1 else dict(onehot=n_b, dyadic=n_b, general=n_b)
        return {k: v * n_a * n_b for k, v in per.items()}

    # K(x, y) by the twin and in closed form, [a, b] with A in the x role and [b, a] with B in it
    ref_ab = np.array([[po.si_str_ld(a, b, g, 1.0, 0.0) for b in ob] for a in oa])
    ref_ba = np.array([[po.si_str_ld(b, a, g, 1.0, 0.0) for a in oa] for b in ob])
    cf = np.array([[1.0 + gp[pa[0] + pb[0] - 2] for _, pb in SHORT_Y] for _, pa in LONG_X])
    if kind == "all3":
        cf[2] = 1.0 + sg.THIRD * (cf[2] - 1.0)   # the probe letter V
    tol = sg.tol_matrix([L for L, _ in LONG_X], [L for L, _ in SHORT_Y])
    assert np.all(np.abs(ref_ab - cf) <= tol * cf) and np.all(np.abs(ref_ba - cf.T) <= tol.T * cf.T)
    assert np.all(ref_ab - 1.0 >= 100 * tol)

    def ran_is(w, ymax):  # ymax: the longest example of the y set, which sizes the kernels' LDS rows
        counts, waves = sg.ran(gpu_ctx)
        if w is not None:
            assert counts == w, (counts, w)
        else:  # one example of the mixed set: one kernel took the row
            assert sorted(counts.values())[:2] == [0, 0] and sum(counts.values()) == nb, counts
        model = dict(onehot=sg.fast_waves(ymax, True), dyadic=sg.fast_waves(ymax, False), general=sg.general_waves(ymax))
        assert all(waves[k] == (model[k] if counts[k] else 0) for k in counts), (waves, model)

    la, lb = max(L for L, _ in LONG_X), max(L for L, _ in SHORT_Y)
    # test_matrix(test, train)[t, j] = K(x = train[j], y = test[t])
    m, _ = gpu_ctx.test_matrix(B, A, kern)          # the x set longer than every y
    ran_is(want(na, nb), lb)
    _check(f"two sets {kind} gap {g}: matrix, long x", m, ref_ab.T, tol.T)
    m, _ = gpu_ctx.test_matrix(A, B, kern)          # the y set longer than every x
    ran_is(want(na, nb), la)
    _check(f"two sets {kind} gap {g}: matrix, long y", m, ref_ba.T, tol)
    for t in range(nb):                             # row t of B against A in the x role
        r = gpu_ctx.test_row(B, t, A, kern)
        ran_is(want(na, 1), lb)
        _check(f"two sets {kind} gap {g}: row {t}, long x", r, ref_ab[:, t], tol[:, t])
    for t in range(na):                             # row t of A against B in the x role
        r = gpu_ctx.test_row(A, t, B, kern)
        ran_is(want(1, nb), la)
        _check(f"two sets {kind} gap {g}: row {t}, long y", r, ref_ba[:, t], tol[t])
