"""Shared child sums of the DAG stem kernel's gamma schedule (DESIGN.md 3.7,
host/pack_shared_sums.cpp): a set of children that several swept x rows read
becomes one combination row, and each of those rows reads it in place of the
set.  The kernel runs the factored schedule by default; here it is checked on
every ordered pair of each set

  - against the C oracle at the tolerance tests/test_gamma.py uses for it
    (1e-6 relative), and
  - against the plain gamma schedule (experiments build, SK_NO_SHARED_SUMS
    read when a dataset is packed) at 1e-12 relative: the factoring only
    reassociates sums of positive terms, a few ulp per level.

Sets: 8 sequences at L = 60 and 6 at L = 120 (register classes MAXK 8 and
12 / 16 with the synthetic fold; 6 at L = 40 are added for MAXK 4), 4 at
L = 200 taken from the config-size fixtures by node count for MAXK 16, 17
and 20, the L = 60 set without a length band, and the mixed inputs of
tests/test_gamma.py, whose gapped alignment makes its y pairs run the full
schedule (no Gamma tables for that y).  Every test asserts through
sk_dataset_shared_sums that its x examples have shared-sum rows, and through
sk_last_classes which register classes ran.

The *_long_gaps tests repeat both comparisons at loop_gap 0.98, the first
against the long-double oracle at the derived tolerance of
tests/stem_long_gaps.py (measured on an MI355X: max relative
error 3.3e-15 at L = 200, 7e-4 of the tolerance)."""
import os

import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem_long_gaps as slg
from tests.helpers import make_examples, mutate_alignment, rel_err

LONG_GAP = slg.LONG_GAP

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 0x55A0


def _maxk(nl):  # tests/test_large_configs.py
    s = (nl + 1 + 63) // 64
    return 17 if s == 17 else (s + 3) // 4 * 4


def _l200():
    dag = np.load(os.path.join(GOLDEN, "large_dag.npz"))
    seqs = [str(s) for name in ("ns_L200", "ns20_L200") for s in dag[f"{name}_seqs"]]
    nl = [int(np.sum(ska.Dataset.synthetic([s]).dag(0)["n_edges"] > 0)) for s in seqs]
    pick = []
    for k in (16, 17, 20, 20):  # one per class, a second MAXK 20 y
        pick.append(next(i for i in range(len(seqs)) if _maxk(nl[i]) == k and i not in pick))
    return [seqs[i] for i in pick]


def _mixed(seed):  # tests/test_gamma.py _inputs: items 2 is a gapped alignment
    base = ska.random_sequences(4, 64, seed)
    return [base[0], mutate_alignment(base[1], 3, seed + 1, gap=0.0), mutate_alignment(base[2], 2, seed + 2),
            base[3], mutate_alignment(base[0], 2, seed + 3, gap=0.0)]


# name -> (items, kernel, classes that must run, x examples that must have shared sums)
def _cases():
    l60 = ska.random_sequences(8, 60, SEED + 60)
    return {
        "L40": (ska.random_sequences(6, 40, SEED + 40), ska.SuStemKernel(loop_gap=0.4), {4}, None),
        "L60": (l60, ska.SuStemKernel(loop_gap=0.4), {8}, None),
        "L120": (ska.random_sequences(6, 120, SEED + 120), ska.SuStemKernel(loop_gap=0.4), {12}, None),
        "L200": (_l200(), ska.SuStemKernel(), {16, 17, 20}, None),
        "band0": (l60, ska.SuStemKernel(loop_gap=0.4, len_band=0), {8}, None),
        "gapped_y": (_mixed(0x6A44A), ska.SuStemKernel(loop_gap=0.4, len_band=4), set(), [0, 3]),
    }


CASES = ["L40", "L60", "L120", "L200", "band0", "gapped_y"]


@pytest.fixture(scope="module")
def cases():
    return _cases()


def _pairs(ctx, items, kern, switch=None):
    """(all ordered pairs as an n x n matrix, the dataset, the oracle's examples), the dataset packed with
    `switch` set"""
    saved = os.environ.pop("SK_NO_SHARED_SUMS", None)
    try:
        if switch:
            os.environ["SK_NO_SHARED_SUMS"] = "1"
        ds, om = make_examples(items)
        n = len(items)
        x, y = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
        return ctx.pairs(ds, kern, x, y).reshape(n, n), ds, om
    finally:
        os.environ.pop("SK_NO_SHARED_SUMS", None)
        if saved is not None:
            os.environ["SK_NO_SHARED_SUMS"] = saved


def _assert_shared(ds, n, which):
    counts = [ds.shared_sums(i) for i in range(n)]
    print("shared-sum rows, member records replaced:", counts)
    for i in (which if which is not None else range(n)):
        assert counts[i][0] > 0 and counts[i][1] >= 2 * counts[i][0], (i, counts)


@pytest.mark.parametrize("name", CASES)
def test_shared_sums_oracle(gpu_ctx, cases, name):
    items, kern, classes, which = cases[name]
    got, ds, om = _pairs(gpu_ctx, items, kern)
    ran = set(gpu_ctx.last_classes()["stem_maxk"])
    n = len(items)
    _assert_shared(ds, n, which)
    p = kern.params
    ref = np.array([[po.su_stem(om[i], om[j], p.loop_gap, p.beta, p.len_band) for j in range(n)] for i in range(n)])
    err = rel_err(got, ref)
    print(f"{name}: classes {sorted(ran)}, max rel err {err:.3g}")
    assert classes <= ran, (classes, ran)
    assert err < 1e-6


def _long(kern):
    return ska.SuStemKernel(loop_gap=LONG_GAP, len_band=kern.params.len_band)


@pytest.mark.parametrize("name", CASES)
def test_shared_sums_oracle_long_gaps(gpu_ctx, cases, name):
    """The same sets at loop_gap 0.98 against the long-double oracle, at the
    derived tolerance of tests/stem_long_gaps.py."""
    items, kern, classes, which = cases[name]
    kern = _long(kern)
    got, ds, om = _pairs(gpu_ctx, items, kern)
    ran = set(gpu_ctx.last_classes()["stem_maxk"])
    _assert_shared(ds, len(items), which)
    worst, err, tol = slg.su_excess(got, om, om, kern)
    print(f"{name}, loop_gap {LONG_GAP}: classes {sorted(ran)}, max rel err {err:.3g}, err / tolerance {worst:.3g} "
          f"(tolerance <= {tol:.3g})")
    assert classes <= ran, (classes, ran)
    assert tol <= slg.TOL_CAP
    assert worst <= 1.0


@pytest.mark.explib
@pytest.mark.parametrize("name", CASES)
def test_shared_sums_equal_plain_schedule_long_gaps(gpu_ctx, cases, name):
    items, kern, _, which = cases[name]
    kern = _long(kern)
    on, ds_on, _ = _pairs(gpu_ctx, items, kern)
    off, ds_off, _ = _pairs(gpu_ctx, items, kern, switch=True)
    n = len(items)
    _assert_shared(ds_on, n, which)
    assert all(ds_off.shared_sums(i) == (0, 0) for i in range(n))
    err = rel_err(on, off)
    print(f"{name}, loop_gap {LONG_GAP}: factored against plain, max rel err {err:.3g}")
    assert err < 1e-12


@pytest.mark.explib
@pytest.mark.parametrize("name", CASES)
def test_shared_sums_equal_plain_schedule(gpu_ctx, cases, name):
    items, kern, _, which = cases[name]
    on, ds_on, _ = _pairs(gpu_ctx, items, kern)
    off, ds_off, _ = _pairs(gpu_ctx, items, kern, switch=True)
    n = len(items)
    _assert_shared(ds_on, n, which)
    assert all(ds_off.shared_sums(i) == (0, 0) for i in range(n))  # the switch selects the plain schedule
    rows_on = sum(ds_on.row_traffic(i)["rows"] for i in range(n))
    rows_off = sum(ds_off.row_traffic(i)["rows"] for i in range(n))
    assert rows_on > rows_off
    err = rel_err(on, off)
    print(f"{name}: factored against plain, max rel err {err:.3g}")
    assert err < 1e-12
