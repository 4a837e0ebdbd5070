"""Conditions on the inputs of the 4-D kernels' probe tests
(tests/test_stem4d_probes.py), checked on the CPU: every probe's targeted
term is a visible share of K at the gaps it runs at; the blind spot of gap
0.8 and of the dense square sets, which is why those gaps and the sparse and
lopsided inputs are there; a truncated base-term table fails the probes by
orders of magnitude; and every tolerance the GPU tests use is under its cap.
DESIGN.md §7.3."""
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem4d_probes as sp


@pytest.mark.parametrize("family", sp.FAMILIES)
def test_every_probe_sees_its_term(family):
    """At each of its gaps: removing the targeted inner pair changes K by at
    least 1e-3 relative ((K - 1) / K for the table-end probes), and so do the
    terms that reach the pair across the run alone -- except where the probe
    is the variant whose inner G3 source must not fire (no such term)."""
    low = 1.0
    for pr in sp.probes(family):
        for g in sp.probe_gaps(pr):
            s = sp.share(pr, g)
            assert s >= sp.SHARE, (pr.name, g, s)
            low = min(low, s)
            if pr.target:
                s = sp.share(pr, g, nested_only=True)
                if pr.name.endswith("inner_subst"):
                    assert s == 0.0, (pr.name, g, s)
                else:
                    assert s >= sp.SHARE, (pr.name, g, s)
                    low = min(low, s)
    print(f"{family}: smallest share {low:.3g}")


@pytest.mark.parametrize("family", sp.FAMILIES)
def test_gap_08_is_blind_to_long_runs(family):
    """The blind spot, recorded: at the default gap 0.8 the terms that cross
    a run of 64 or more skipped positions are below the older tests' 1e-6 on
    the very same probes."""
    seen = 0
    for pr in sp.probes(family):
        if pr.run < 64 or pr.name.endswith("inner_subst"):
            continue
        s = sp.share(pr, sp.DEFAULT_GAP, nested_only=True)
        assert 0.0 < s < sp.BLIND, (pr.name, s)
        seen += 1
    assert seen >= 1   # (the seam family has one such run, the 1,000 across both seams)


def _cut_change(xa, xb, gap, cut):
    a = (xa.lower(), sp.folded(xa), xb.lower(), sp.folded(xb), sp.f32(gap))
    full = po.stem4d_gen(*a)
    return abs(po.stem4d_gen(*a, cut=cut) - full) / full


def test_dense_square_pair_is_blind_to_truncated_base_terms():
    """The blind spot, recorded: on the suite's dense L = 70 pair a kernel
    whose base terms g^(l-k) and g^(j-i) end after 32 positions moves K by
    less than 1e-6 at gap 0.8 (6.8e-7), and cut after 48 positions it stays
    below 1e-6 even at gap 1.0; the lopsided 24 x 300 pair sees the same
    cut-off at 48 well above 1e-6 at gap 0.98."""
    s = ska.random_sequences(2, 70, 0x5EED0013)
    c = _cut_change(s[0], s[1], 0.8, 32)
    assert 1e-8 < c < sp.BLIND, c
    assert _cut_change(s[0], s[1], 1.0, 48) < sp.BLIND
    seqs, pairs = sp.dense_set("lop")
    lop = _cut_change(seqs[pairs[0][0]], seqs[pairs[0][1]], 0.98, 48)
    print(f"cut 32 at L = 70, gap 0.8: {c:.3g}; cut 48 at 24 x 300, gap 0.98: {lop:.3g}")
    assert lop > 1e-3


def _long_in_y(pr):
    return pr if len(pr.y) >= len(pr.x) else sp.exchanged(pr)


@pytest.mark.parametrize("family", sp.FAMILIES)
def test_truncated_table_fails_the_probes(family):
    """A reference with the base terms cut off after 48 positions (the twin's
    cut argument) misses the closed form by more than 1e6 tolerances on every
    table-end and long-run probe, that is, wherever a pair of the long
    sequence spans more than 64 positions (the seam probes' short pairs next
    to a seam hold no such term).  The cut-off is on y spans (and on the
    diagonal cells' x spans), so a probe with its run in x is evaluated with
    x and y exchanged."""
    seen = 0
    for pr in sp.probes(family, small=True):
        q = _long_in_y(pr)
        if max(b - a for a, b, _ in q.yp) <= 64:
            continue
        g = sp.probe_gaps(q)[0]
        cf = float(sp.closed_form(q, g))
        assert abs(float(sp.closed_form(pr, g)) - cf) <= 1e-15 * cf   # K is symmetric in x and y
        err = abs(sp.twin_of_probe(q, g, cut=48) - cf) / cf
        assert err > 1e6 * sp.probe_tol(q), (pr.name, err)
        seen += 1
    assert seen >= 3


def test_tolerances_under_their_caps():
    """Every tolerance of tests/test_stem4d_probes.py, from the formula alone."""
    top = 0.0
    for family in sp.FAMILIES:
        for pr in sp.probes(family):
            for banded in (False, True):
                top = max(top, sp.probe_tol(pr, banded))
                assert sp.probe_tol(pr, banded) <= sp.PROBE_CAP, pr.name
    dense = 0.0
    for name in sp.DENSE_SETS + ("col", "tiled"):
        seqs, pairs = sp.dense_set(name)
        for band in sp.DENSE_BANDS + (sp.TILED_BAND,):
            t = sp.pair_tols(seqs, pairs, ska.StemKernel4D(band=band).params).max()
            assert t <= sp.DENSE_CAP, (name, band, t)
            dense = max(dense, t)
    print(f"largest tolerance: probes {top:.3g}, dense {dense:.3g}")


def _suite_twin_cases():
    """(sequences, pairs, kernel) of every twin comparison of
    tests/test_stem4d.py, with its bp models, bounds, loops and bands (S is
    largest under NormalBasePair / WobbleBasePair, where every canonical pair
    beyond the loop counts)."""
    gram = lambda s: [(a, b) for a in range(len(s)) for b in range(a, len(s))]
    s = sp.suite_seqs()
    for model, bound in [(0, 0.0), (0, 0.3), (1, 0.5), (2, 0.5), (1, 1.0)]:
        yield s, gram(s), ska.StemKernel4D(bp_model=model, bp_bound=bound)
    s = list(sp.dense_set("col")[0])
    yield s, gram(s), ska.StemKernel4D()
    s = ska.random_sequences(5, 40, 0x5EED0033)
    yield s, gram(s), ska.StemKernel4D(gap=0.5, stack=1.5, subst=0.25, loop=4)
    tr = ska.random_sequences(4, 45, 0x5EED0051) + ["GGGGAAAACCCC"]
    te = ska.random_sequences(3, 70, 0x5EED0052)
    for kern in [ska.StemKernel4D(bp_model=1, bp_bound=0.5), ska.StemKernel4D(),
                 ska.StemKernel4D(bp_model=2, bp_bound=0.5, loop=5)]:
        yield te + tr, [(a, len(te) + b) for a in range(len(te)) for b in range(len(tr))], kern
    s = list(sp.dense_set("lop")[0])
    yield s, [(a, b) for a in range(3) for b in (3, 4)], ska.StemKernel4D(bp_model=2, bp_bound=0.3)
    ys = ["GC", "GCU", "GGCC", "GAUCA", "GGAUCC", "GGGAUCC", "GCGAAAGC"]
    xs = ska.random_sequences(3, 16, 0x5EED0071) + ["GGGGAAACCCC"]
    yield xs + ys, [(a, len(xs) + b) for a in range(len(xs)) for b in range(len(ys))], \
        ska.StemKernel4D(bp_model=2, bp_bound=0.3)
    s = ska.random_sequences(3, 40, 0x5EED0043) + ska.random_sequences(2, 27, 9)
    s += ska.random_sequences(1, 70, 10) + ["GGGAAACCC", "A"]
    for band in (1, 3, 8, 100):
        yield s, [(a, b) for a in range(len(s)) for b in range(len(s))], ska.StemKernel4D(band=band)


def test_suite_tolerances_under_the_cap():
    """The derived tolerances tests/test_stem4d.py compares at (its
    _twin_check asserts the same cap on what it actually runs)."""
    top = 0.0
    for seqs, pairs, kern in _suite_twin_cases():
        t = sp.pair_tols(seqs, pairs, kern.params).max()
        assert t <= sp.DENSE_CAP, (kern.params.bp_model, kern.params.bp_bound, kern.params.len_band, t)
        top = max(top, t)
    print(f"largest tolerance of tests/test_stem4d.py: {top:.3g}")


def test_seam_run_passes_through_the_middle_tile():
    """The seam family's long run: outer k in the first k tile, inner k in
    the third, so its chain crosses both seams (and likewise scaled down)."""
    for small, (s0, s1) in ((False, (512, 1024)), (True, (64, 128))):
        pr = next(p for p in sp.probes("seam", small) if p.name.startswith("se_run"))
        (ko, _, _), (ki, _, _) = pr.yp
        assert ko < s0 and ki >= s1 and pr.run == ki - ko - 1 and pr.target == ("y", (ki, pr.yp[1][1]))
    assert pr.run == 120 and next(p for p in sp.probes("seam") if p.name == "se_run1000").run == 1000


def test_tiled_banded_pair_crosses_the_seam():
    """The banded pair over k tiles: |x| <= 24, |y| >= 1,040, and the band's
    windows [c_low, c_high] hold k = 512 for at least three values of i."""
    import numpy as np
    seqs, _ = sp.dense_set("tiled")
    n, m = len(seqs[0]), len(seqs[1])
    assert n <= 24 and m >= 1040
    lo, hi = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
    po.oracle().orc_stem4d_band(n, m, sp.TILED_BAND, lo.ctypes.data_as(po._U), hi.ctypes.data_as(po._U))
    assert int(np.sum((lo <= 512) & (512 <= hi))) >= 3
