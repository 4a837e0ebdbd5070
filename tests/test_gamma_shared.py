"""Shared Gamma tables of the DAG stem kernel (dag_stem.hip):
a table kernel builds one Gamma table per gapless y of a class launch and
every workgroup on that y reads it.  The Gram must match the oracle with one
table read by several workgroups (the grid shrinks to the item count) and a
gapped y that has no table; with separate row and column sets (the keys
come from the x set); and the per-workgroup tables a launch falls back to
beyond the memory budget must give the same bits (experiments build:
SK_GAM_TABLE_MB; runs under tests/test_explib.py).

The *_long_gaps tests repeat these at loop_gap 0.98, where the edges of more
than a dozen skipped positions reach the compared digits, against the
long-double oracle at the derived tolerance of tests/stem_long_gaps.py
(measured on an MI355X: max relative error 1.2e-15, 1.1e-3
of the tolerance)."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem_long_gaps as slg
from tests.helpers import make_examples, mutate_alignment, rel_err
from tests.test_gamma import _inputs

pytestmark = pytest.mark.gpu

LONG_GAP = slg.LONG_GAP


def _path_inputs(seed):
    """36 single sequences of L = 48 and the five mixed inputs of
    tests/test_gamma.py: every y has a column of up to 41 pairs, three or more
    one-round items that different workgroups take."""
    return ska.random_sequences(36, 48, seed) + _inputs(seed + 1)


@pytest.mark.parametrize("band", [0, 4])
def test_shared_tables_oracle(gpu_ctx, band):
    items = _path_inputs(0x6A5E0 + band)
    kern = ska.SuStemKernel(loop_gap=0.4, len_band=band)
    ds, om = make_examples(items)
    got = gpu_ctx.gram(ds, kern)
    shared = gpu_ctx.last_gamma_shared()
    n = len(items)
    ref = np.array([[po.su_stem(om[i], om[j], 0.4, kern.params.beta, band) if j >= i else 0.0
                     for j in range(n)] for i in range(n)])
    ref = np.triu(ref) + np.triu(ref, 1).T
    err = rel_err(got, ref)
    print(f"band {band}: shared launches {shared}, max rel err {err:.3g}")
    assert shared > 0
    assert err < 1e-6


def test_shared_tables_row_and_column_sets(gpu_ctx):
    """The keys are the row (x) set's; the tables are built of the column
    set's y's."""
    train, om = make_examples(_inputs(0x6A5F0))
    test, omt = make_examples([ska.random_sequences(1, 70, 0x6A5F1)[0],
                               mutate_alignment(ska.random_sequences(1, 66, 0x6A5F2)[0], 2, 3, gap=0.0)])
    kern = ska.SuStemKernel()
    for t in range(2):
        row = gpu_ctx.test_row(test, t, train, kern)
        assert gpu_ctx.last_gamma_shared() > 0
        ref = [po.su_stem(om[x], omt[t]) for x in range(len(om))]
        assert rel_err(row, ref) < 1e-6


@pytest.mark.explib
@pytest.mark.parametrize("band", [0, 4])
def test_per_workgroup_fallback_agrees(gpu_ctx, band, monkeypatch):
    """Budget 0: every launch builds its tables per workgroup and item, by the
    same code as the table kernel (bit equality expected; bound: the 1e-14
    of test_gamma_switches_agree's SK_STORE_ALL)."""
    items = _path_inputs(0x6A5E0 + band)
    kern = ska.SuStemKernel(loop_gap=0.4, len_band=band)
    ds, _ = make_examples(items)
    monkeypatch.delenv("SK_GAM_TABLE_MB", raising=False)
    on = gpu_ctx.gram(ds, kern)
    assert gpu_ctx.last_gamma_shared() > 0
    monkeypatch.setenv("SK_GAM_TABLE_MB", "0")
    off = gpu_ctx.gram(ds, kern)
    assert gpu_ctx.last_gamma_shared() == 0
    monkeypatch.delenv("SK_GAM_TABLE_MB")
    err = rel_err(on, off)
    print(f"band {band}: shared vs per-workgroup tables: max rel err {err:.3g}, equal {np.array_equal(on, off)}")
    assert err < 1e-14


@pytest.mark.parametrize("band", [0, 4])
def test_shared_tables_oracle_long_gaps(gpu_ctx, band):
    items = _path_inputs(0x6A5E0 + band)
    kern = ska.SuStemKernel(loop_gap=LONG_GAP, len_band=band)
    ds, om = make_examples(items)
    got = gpu_ctx.gram(ds, kern)
    shared = gpu_ctx.last_gamma_shared()
    worst, err, tol = slg.su_excess(got, om, om, kern, upper=True)
    print(f"band {band}: shared launches {shared}, max rel err {err:.3g}, err / tolerance {worst:.3g} (tolerance <= {tol:.3g})")
    assert shared > 0
    assert np.array_equal(got, got.T)
    assert tol <= slg.TOL_CAP
    assert worst <= 1.0


def test_shared_tables_row_and_column_sets_long_gaps(gpu_ctx):
    train, om = make_examples(_inputs(0x6A5F0))
    test, omt = make_examples([ska.random_sequences(1, 70, 0x6A5F1)[0],
                               mutate_alignment(ska.random_sequences(1, 66, 0x6A5F2)[0], 2, 3, gap=0.0)])
    kern = ska.SuStemKernel(loop_gap=LONG_GAP)
    for t in range(2):
        row = gpu_ctx.test_row(test, t, train, kern)
        assert gpu_ctx.last_gamma_shared() > 0
        worst, err, tol = slg.su_excess(row, om, [omt[t]], kern)
        print(f"test {t}: max rel err {err:.3g}, err / tolerance {worst:.3g} (tolerance <= {tol:.3g})")
        assert tol <= slg.TOL_CAP
        assert worst <= 1.0


@pytest.mark.explib
@pytest.mark.parametrize("band", [0, 4])
def test_per_workgroup_fallback_agrees_long_gaps(gpu_ctx, band, monkeypatch):
    items = _path_inputs(0x6A5E0 + band)
    kern = ska.SuStemKernel(loop_gap=LONG_GAP, len_band=band)
    ds, _ = make_examples(items)
    monkeypatch.delenv("SK_GAM_TABLE_MB", raising=False)
    on = gpu_ctx.gram(ds, kern)
    assert gpu_ctx.last_gamma_shared() > 0
    monkeypatch.setenv("SK_GAM_TABLE_MB", "0")
    off = gpu_ctx.gram(ds, kern)
    assert gpu_ctx.last_gamma_shared() == 0
    monkeypatch.delenv("SK_GAM_TABLE_MB")
    err = rel_err(on, off)
    print(f"band {band}, loop_gap {LONG_GAP}: shared vs per-workgroup tables: max rel err {err:.3g}")
    assert err < 1e-14
