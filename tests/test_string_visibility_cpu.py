"""Where the string kernels' GPU tests (tests/test_string_long_gaps.py) can
fail: each case recomputed on the CPU with the table twin of the string DP
(oracle/sk_oracle.c: orc_profile_string_tab, orc_naive_string_tab) at the
case's own parameters, with one bucket of its four tables zeroed:

  C[64..]    G0[i][0], i >= 64: column 0's gap powers beyond the first strip
  R[64..]    G0[0][j], j >= 64: the row-0 boundary beyond column 63
  wh[a..b]   horizontal runs of a..b skipped columns (13-32, 33-64, >= 65)
  wv[a..b]   vertical runs of a..b skipped rows, likewise

and the relative change of K divided by the case's GPU tolerance.  A kernel
that loses a bucket's terms fails a case whose figure is well above 1; the
sparse probes must reach 100 in every bucket, and do; the dense sets reach it
only in the short-run buckets, which is why the probes exist.  The figures
are tabulated in DESIGN.md §7.2.  CPU only.
"""
import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem_long_gaps as slg
from tests import string_long_gaps as sg
from tests.helpers import make_examples

NX1 = len(sg.X_SINGLE)
# bucket -> the probe pairs meant to see it, as indices into a probe set (x side first: singles, then doubles)
_xs = {p: k for k, p in enumerate(sg.X_SINGLE)}
_ys = {p: sg.N_X + k for k, p in enumerate(sg.Y_SINGLE)}
_run = {r: k for k, r in enumerate(sg.RUNS)}


def _dbl(run):
    return NX1 + _run[run], sg.N_X + len(sg.Y_SINGLE) + _run[run]


DESIGNATED = {
    ("C", 64, None): [(_xs[(193, (129,))], _ys[(200, (1,))]), (_xs[(193, (193,))], _ys[(5, (1,))])],
    ("R", 64, None): [(_xs[(1, (1,))], _ys[(200, (129,))]), (_xs[(65, (1,))], _ys[(200, (200,))])],
    ("wh", 13, 32): [_dbl((1, 20))],
    ("wh", 33, 64): [_dbl((1, 62)), _dbl((60, 64))],
    ("wh", 65, None): [_dbl((1, 127)), _dbl((60, 65))],
    ("wv", 13, 32): [_dbl((1, 20))],
    ("wv", 33, 64): [_dbl((1, 62)), _dbl((60, 64))],
    ("wv", 65, None): [_dbl((1, 127)), _dbl((60, 65))],
}


def _probe_tab(variant, om, first, a, b, g):
    if sg.VARIANTS[variant][5]:
        return lambda tab: po.naive_string_tab(first[a], first[b], g, tab)
    return lambda tab: po.si_str_tab(om[a], om[b], tab, 1.0, 0.0)


@pytest.mark.parametrize("variant,use_bp", [(v, bp) for v in sg.VARIANTS for bp in (False, True)
                                            if not (v == "mixed" and not bp)])
def test_probes_see_every_bucket(variant, use_bp):
    ds, om, first, lens, hw = sg.probe_set(variant, use_bp)
    naive = sg.VARIANTS[variant][5]
    tol = sg.probe_tol(lens, sg.categories(ds, hw), naive)
    for g in sg.GAPS:
        line = []
        for bucket in sg.BUCKETS:
            best = 0.0
            for a, b in DESIGNATED[bucket]:
                ch = sg.masked_change(_probe_tab(variant, om, first, a, b, g), g, lens[a], lens[b], bucket)
                best = max(best, ch / tol[a, b])
            line.append(f"{sg.bucket_name(bucket)} {best:.2g}")
            assert best >= 100.0, (variant, use_bp, g, bucket, best)
        print(f"probes {variant} use_bp {use_bp} gap {g}: change / tolerance  " + "  ".join(line))


def test_probe_matrix():
    """Every designated pair against every bucket (one-hot, unweighted): what
    each probe sees and what it does not (printed; the diagonal is asserted
    above)."""
    ds, om, first, lens, hw = sg.probe_set("onehot", False)
    tol = sg.probe_tol(lens, sg.categories(ds, hw))
    pairs = sorted({p for v in DESIGNATED.values() for p in v})
    pos = sg.probe_positions()
    for g in sg.GAPS:
        for a, b in pairs:
            f = _probe_tab("onehot", om, first, a, b, g)
            row = [sg.masked_change(f, g, lens[a], lens[b], bk) / tol[a, b] for bk in sg.BUCKETS]
            print(f"gap {g} x {lens[a]}:{pos[a]} y {lens[b]}:{pos[b]}  " +
                  "  ".join(f"{sg.bucket_name(bk)} {v:.2g}" for bk, v in zip(sg.BUCKETS, row)))


# the dense sets' pairs: two of lengths 129 / 193 / 200 per set, and L = 300 x 300 for the singles
def _dense_pairs(name, lens):
    k = {L: i for i, L in enumerate(lens)}
    p = [(k[129], k[200]), (k[193], k[129])]
    return p + [(lens.index(300), lens.index(300) + 1)] if name == "single" else p


@pytest.mark.parametrize("name", sg.DENSE_SETS)
def test_dense_sets_see_the_short_runs(name):
    ds, om, lens, hw = sg.dense_set(name)
    tol = sg.probe_tol(lens, sg.categories(ds, hw))
    for which in sg.DENSE_KERNELS:
        for g in sg.DENSE_GAPS:
            f = (lambda a, b: lambda tab: po.su_str_tab(om[a], om[b], tab, sg.ALPHA)) if which == "su" else \
                (lambda a, b: lambda tab: po.si_str_tab(om[a], om[b], tab, sg.MATCH, sg.MISMATCH))
            best = {}
            for a, b in _dense_pairs(name, lens):
                for bucket in sg.BUCKETS:
                    ch = sg.masked_change(f(a, b), g, lens[a], lens[b], bucket) / tol[a, b]
                    best[bucket] = max(best.get(bucket, 0.0), ch)
            print(f"dense {name} {which} gap {g}: change / tolerance  " +
                  "  ".join(f"{sg.bucket_name(bk)} {best[bk]:.2g}" for bk in sg.BUCKETS))
            # what the dense sets are meant to see: runs of 13-32 in both directions at every gap
            assert best[("wh", 13, 32)] >= 100.0 and best[("wv", 13, 32)] >= 100.0, (name, which, g, best)


@pytest.mark.parametrize("name", list(slg.CLASS_SETS))
def test_sum_kinds_see_both_parts(name):
    """Kinds 4, 5 and 7: the relative error of the stem part and of the
    string part that the GPU test's allowed error would still catch (the
    smallest over the set's pairs), per (loop_gap, band); and the string
    buckets through kind 7's string term for one pair."""
    ds, om, st = slg.built(name)
    lens = [po.oracle().orc_mdata_seq_len(o.h) for o in om]
    tol_stem, tol_str = slg.tol_matrix(st), sg.tol_matrix(lens, path="onehot")
    k2, k3 = sg.sum_string_reference(name)
    for g, band in sg.SUM_PARAMS:
        ref = slg.reference(name, g, band)
        for kind in (4, 5, 7):
            p = slg.kernel(kind, g, band).params
            stem, s = (ref["si"], k3) if kind == 5 else (ref["su"], k2)
            _, allowed = sg.sum_allowed(kind, stem, s, tol_stem, tol_str, p)
            if kind == 7:
                see_stem, see_str = allowed / abs(p.beta), allowed / abs(p.alpha)
            else:
                see_stem, see_str = allowed / stem, allowed / s
            print(f"{name} loop_gap {g} band {band} kind {kind}: smallest relative error caught, stem "
                  f"{see_stem.min():.2g} .. {see_stem.max():.2g}, str {see_str.min():.2g} .. {see_str.max():.2g}; "
                  f"stem / str {np.min(stem / s):.2g} .. {np.max(stem / s):.2g}")
            if kind == 7:  # both parts within ten ceilings: the case that matters
                assert see_stem.max() <= 10 * sg.TOL_CAP and see_str.max() <= 10 * sg.TOL_CAP
    if lens[0] <= 300:
        p = ska.LSuStemStrKernel().params
        a, b = 0, 1
        tol7 = (abs(p.beta) * tol_stem[a, b] + abs(p.alpha) * tol_str[a, b]) / abs(p.alpha)
        f = lambda tab: po.su_str_tab(om[a], om[b], tab, p.alpha)
        print(f"{name} kind 7, string gap {p.gap}: change of the string term / allowed  " + "  ".join(
            f"{sg.bucket_name(bk)} {sg.masked_change(f, p.gap, lens[a], lens[b], bk) / tol7:.2g}"
            for bk in sg.BUCKETS))


def test_existing_fixture_at_the_old_tolerance():
    """For comparison (printed only): a pair of tests/test_string_fast.py's
    L = 150 sequences at its gap 0.8 and the suite's 1e-6."""
    s = ska.random_sequences(6, 150, 0x5EED0B00)
    _, om = make_examples([s[0], s[1]], use_bp=False)
    f = lambda tab: po.su_str_tab(om[0], om[1], tab, 0.2)
    print("test_string_fast L = 150, gap 0.8, tolerance 1e-6: change / tolerance  " + "  ".join(
        f"{sg.bucket_name(bk)} {sg.masked_change(f, 0.8, 150, 150, bk) / 1e-6:.2g}" for bk in sg.BUCKETS))
