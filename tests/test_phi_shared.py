"""Shared Phi tables and the item queues of the DAG stem kernel (dag_stem.hip,
DESIGN.md §4): the table kernel builds, behind a y's Gamma table, one Phi
table per gapless y of a class launch (every phi key of the x set) and every
workgroup on that y reads it; the items of a class launch stand in eight
queues, one per XCD (whole y columns dealt by cost, items capped at a share
of their column), and a workgroup whose queue is empty takes from the others.
The Gram must match the oracle with several workgroups on one table and a
gapped y that has none; with separate row and column sets (the keys come from
the x set); with fewer columns than queues, one column, nine unequal columns,
two register classes in one call and a column shorter than a workgroup's
waves; and the per-workgroup tables (budget 0) and the single queue must give
the same bits (experiments build: SK_GAM_TABLE_MB, SK_PHI_TABLE_MB,
SK_ITEM_QUEUES; run under tests/test_explib.py).

The *_long_gaps tests repeat these at loop_gap 0.98 against the long-double
oracle at the derived tolerance of tests/stem_long_gaps.py (DESIGN.md §7.1;
measured on an MI355X: max relative error 1.8e-15, 1.6e-3 of the tolerance)."""
import functools

import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem_long_gaps as slg
from tests.helpers import make_examples, mutate_alignment, rel_err
from tests.test_gamma import _inputs
from tests.test_gamma_shared import _path_inputs

pytestmark = pytest.mark.gpu

SEED = 0x9B150
LONG_GAP = slg.LONG_GAP


@functools.lru_cache(maxsize=None)
def _path_case(band):
    """The path inputs, their dataset and the oracle's whole matrix
    ref[x, y] (computed once per band, shared, never written)."""
    items = _path_inputs(SEED + band)
    ds, om = make_examples(items)
    kern = ska.SuStemKernel(loop_gap=0.4, len_band=band)
    n = len(items)
    ref = np.array([[po.su_stem(om[i], om[j], 0.4, kern.params.beta, band) for j in range(n)] for i in range(n)])
    ref.setflags(write=False)
    return ds, kern, ref


@functools.lru_cache(maxsize=None)
def _path_case_long(band):
    """_path_case at loop_gap 0.98 (tests/stem_long_gaps.py): the dataset, the
    kernel, the long-double oracle's matrix ref[x, y] (whole for band 0, which
    the queue cases read; x <= y for the others, which only a Gram reads, 1
    elsewhere) and the per-pair tolerance."""
    items = _path_inputs(SEED + band)
    ds, om = make_examples(items)
    kern = ska.SuStemKernel(loop_gap=LONG_GAP, len_band=band)
    st = [slg.dag_stats(o.dag()) for o in om]
    ref = np.array([[po.su_stem_ld(a, b, LONG_GAP, kern.params.beta, band) if band == 0 or j >= i else 1.0
                     for j, b in enumerate(om)] for i, a in enumerate(om)])
    tol = slg.tol_matrix(st)
    assert tol.max() <= slg.TOL_CAP
    ref.setflags(write=False)
    tol.setflags(write=False)
    return ds, kern, ref, tol


def _excess(got, ref, tol):
    return float(np.max(np.abs(got - ref) / (tol * ref)))


def _phi_reads(ds):
    return sum(ds.row_traffic(i)["phi_reads"] for i in range(len(ds)))


@pytest.mark.parametrize("band", [0, 4])
def test_shared_phi_tables_oracle(gpu_ctx, band):
    """Columns of up to 41 pairs: several one-round items, taken by different
    workgroups, read one y's tables; the gapped y has none."""
    ds, kern, ref = _path_case(band)
    got = gpu_ctx.gram(ds, kern)
    shared = gpu_ctx.last_gamma_shared()
    up = np.triu_indices(len(ds))
    err = rel_err(got[up], ref[up])
    print(f"band {band}: shared launches {shared}, phi reads {_phi_reads(ds)}, max rel err {err:.3g}")
    assert shared > 0
    assert _phi_reads(ds) > 0
    assert err < 1e-6


def test_shared_phi_tables_row_and_column_sets(gpu_ctx):
    """The phi keys are the row (x) set's; the tables are built of the column
    set's y's."""
    train, om = make_examples(_inputs(SEED + 0x10))
    test, omt = make_examples([ska.random_sequences(1, 70, SEED + 0x11)[0],
                               mutate_alignment(ska.random_sequences(1, 66, SEED + 0x12)[0], 2, 3, gap=0.0)])
    kern = ska.SuStemKernel()
    for t in range(2):
        row = gpu_ctx.test_row(test, t, train, kern)
        assert gpu_ctx.last_gamma_shared() > 0
        assert _phi_reads(train) > 0
        ref = [po.su_stem(om[x], omt[t]) for x in range(len(om))]
        assert rel_err(row, ref) < 1e-6


def _columns(sizes, n):
    """Pairs (x, y): column y = k has its first sizes[k] x's."""
    x = [i for k, c in enumerate(sizes) for i in range(min(c, n))]
    y = [k for k, c in enumerate(sizes) for _ in range(min(c, n))]
    return np.array(x, np.int32), np.array(y, np.int32)


# column sizes over the 41 path inputs (36 single sequences first); a
# workgroup of their class has 12 waves
QUEUE_CASES = {
    "three_columns": [41, 30, 17],                     # fewer columns than queues
    "one_column": [41],                                # one queue in use, the others empty
    "nine_unequal": [41, 41, 36, 13, 12, 5, 2, 1, 1],  # more columns than queues: idle groups take from others
    "short_column": [3, 40],                           # fewer pairs than a workgroup has waves
}


@pytest.mark.parametrize("case", sorted(QUEUE_CASES))
def test_item_queues_oracle(gpu_ctx, case):
    ds, kern, ref = _path_case(0)
    x, y = _columns(QUEUE_CASES[case], len(ds))
    got = gpu_ctx.pairs(ds, kern, x, y)
    err = rel_err(got, ref[x, y])
    print(f"{case}: {x.size} pairs, max rel err {err:.3g}")
    assert err < 1e-6


def test_item_queues_two_classes(gpu_ctx):
    """One call whose y's fall in two register classes (L = 48 and L = 150):
    two launches, each with its own queues and tables."""
    items = ska.random_sequences(14, 48, SEED + 0x20) + ska.random_sequences(3, 150, SEED + 0x21)
    ds, om = make_examples(items)
    kern = ska.SuStemKernel(loop_gap=0.4, len_band=0)
    n = len(items)
    x, y = np.triu_indices(n)
    got = gpu_ctx.pairs(ds, kern, x.astype(np.int32), y.astype(np.int32))
    classes = gpu_ctx.last_classes()["stem_maxk"]
    ref = np.array([po.su_stem(om[i], om[j], 0.4, kern.params.beta, 0) for i, j in zip(x, y)])
    err = rel_err(got, ref)
    print(f"classes {classes}, max rel err {err:.3g}")
    assert len(classes) >= 2
    assert err < 1e-6


@pytest.mark.parametrize("band", [0, 4])
def test_shared_phi_tables_oracle_long_gaps(gpu_ctx, band):
    ds, kern, ref, tol = _path_case_long(band)
    got = gpu_ctx.gram(ds, kern)
    shared = gpu_ctx.last_gamma_shared()
    up = np.triu_indices(len(ds))
    worst = _excess(got[up], ref[up], tol[up])
    print(f"band {band}, loop_gap {LONG_GAP}: shared launches {shared}, phi reads {_phi_reads(ds)}, "
          f"max rel err {rel_err(got[up], ref[up]):.3g}, err / tolerance {worst:.3g}")
    assert shared > 0
    assert _phi_reads(ds) > 0
    assert worst <= 1.0


def test_shared_phi_tables_row_and_column_sets_long_gaps(gpu_ctx):
    train, om = make_examples(_inputs(SEED + 0x10))
    test, omt = make_examples([ska.random_sequences(1, 70, SEED + 0x11)[0],
                               mutate_alignment(ska.random_sequences(1, 66, SEED + 0x12)[0], 2, 3, gap=0.0)])
    kern = ska.SuStemKernel(loop_gap=LONG_GAP)
    for t in range(2):
        row = gpu_ctx.test_row(test, t, train, kern)
        assert gpu_ctx.last_gamma_shared() > 0
        assert _phi_reads(train) > 0
        worst, err, tol = slg.su_excess(row, om, [omt[t]], kern)
        print(f"test {t}, loop_gap {LONG_GAP}: max rel err {err:.3g}, err / tolerance {worst:.3g}")
        assert tol <= slg.TOL_CAP
        assert worst <= 1.0


@pytest.mark.parametrize("case", sorted(QUEUE_CASES))
def test_item_queues_oracle_long_gaps(gpu_ctx, case):
    ds, kern, ref, tol = _path_case_long(0)
    x, y = _columns(QUEUE_CASES[case], len(ds))
    got = gpu_ctx.pairs(ds, kern, x, y)
    worst = _excess(got, ref[x, y], tol[x, y])
    print(f"{case}, loop_gap {LONG_GAP}: {x.size} pairs, max rel err {rel_err(got, ref[x, y]):.3g}, "
          f"err / tolerance {worst:.3g}")
    assert worst <= 1.0


def test_item_queues_two_classes_long_gaps(gpu_ctx):
    items = ska.random_sequences(14, 48, SEED + 0x20) + ska.random_sequences(3, 150, SEED + 0x21)
    ds, om = make_examples(items)
    kern = ska.SuStemKernel(loop_gap=LONG_GAP, len_band=0)
    got = gpu_ctx.gram(ds, kern)
    classes = gpu_ctx.last_classes()["stem_maxk"]
    worst, err, tol = slg.su_excess(got, om, om, kern, upper=True)
    print(f"loop_gap {LONG_GAP}: classes {classes}, max rel err {err:.3g}, err / tolerance {worst:.3g}")
    assert len(classes) >= 2
    assert tol <= slg.TOL_CAP
    assert worst <= 1.0


@pytest.mark.explib
@pytest.mark.parametrize("band", [0, 4])
def test_table_budgets_and_single_queue_agree_long_gaps(gpu_ctx, band, monkeypatch):
    """test_per_workgroup_phi_tables_agree and test_single_queue_agrees at
    loop_gap 0.98, at their bound."""
    ds, _ = make_examples(_path_inputs(SEED + band))
    kern = ska.SuStemKernel(loop_gap=LONG_GAP, len_band=band)
    for k in ("SK_GAM_TABLE_MB", "SK_PHI_TABLE_MB", "SK_ITEM_QUEUES"):
        monkeypatch.delenv(k, raising=False)
    on = gpu_ctx.gram(ds, kern)
    assert gpu_ctx.last_gamma_shared() > 0
    for knob, value in (("SK_GAM_TABLE_MB", "0"), ("SK_PHI_TABLE_MB", "0"), ("SK_ITEM_QUEUES", "1")):
        monkeypatch.setenv(knob, value)
        off = gpu_ctx.gram(ds, kern)
        if knob != "SK_ITEM_QUEUES":
            assert gpu_ctx.last_gamma_shared() == 0
        monkeypatch.delenv(knob)
        err = rel_err(on, off)
        print(f"band {band}, loop_gap {LONG_GAP}: default vs {knob}={value}: max rel err {err:.3g}")
        assert err < 1e-14


@pytest.mark.explib
@pytest.mark.parametrize("band", [0, 4])
def test_per_workgroup_phi_tables_agree(gpu_ctx, band, monkeypatch):
    """Budget 0 for both tables, and for the Phi tables alone: the launches
    build them per workgroup and item by the table kernel's code (bit equality
    expected; bound: the 1e-14 of test_per_workgroup_fallback_agrees)."""
    ds, kern, _ = _path_case(band)
    for k in ("SK_GAM_TABLE_MB", "SK_PHI_TABLE_MB"):
        monkeypatch.delenv(k, raising=False)
    on = gpu_ctx.gram(ds, kern)
    assert gpu_ctx.last_gamma_shared() > 0
    for knob in ("SK_GAM_TABLE_MB", "SK_PHI_TABLE_MB"):
        monkeypatch.setenv(knob, "0")
        off = gpu_ctx.gram(ds, kern)
        assert gpu_ctx.last_gamma_shared() == 0
        monkeypatch.delenv(knob)
        err = rel_err(on, off)
        print(f"band {band}: shared vs {knob}=0: max rel err {err:.3g}, equal {np.array_equal(on, off)}")
        assert err < 1e-14


@pytest.mark.explib
@pytest.mark.parametrize("band", [0, 4])
def test_single_queue_agrees(gpu_ctx, band, monkeypatch):
    """One item queue with uncapped items (the plan before the queues) against
    the eight: a pair is one wave's work from the same tables either way (bit
    equality expected; bound as above)."""
    ds, kern, _ = _path_case(band)
    monkeypatch.delenv("SK_ITEM_QUEUES", raising=False)
    on = gpu_ctx.gram(ds, kern)
    monkeypatch.setenv("SK_ITEM_QUEUES", "1")
    off = gpu_ctx.gram(ds, kern)
    monkeypatch.delenv("SK_ITEM_QUEUES")
    err = rel_err(on, off)
    print(f"band {band}: eight queues vs one: max rel err {err:.3g}, equal {np.array_equal(on, off)}")
    assert err < 1e-14
