"""The long-gap fixtures can fail, and where: on the CPU, with the oracle's
table variant (orc_su_stem_tab / orc_si_stem_tab), every case of the stem
kernels' long-gap tests is recomputed, at its own loop_gap and its own
len_band, with the gap weights of one bucket zeroed -- buckets 13-32, 33-128,
129-1,023 and >= 1,024, each where the fixture's DAGs hold such an edge -- and,
where it has a band, against the band off.  Each must move at least one
compared value by 100 times that pair's tolerance (tests/stem_long_gaps.py:
4 D 2^-53) or more: a kernel that dropped or misread those edges, or ignored
the band, fails that GPU case by that factor.

Not every case sees every bucket, and the exceptions are written down here and
not asserted at another configuration: with a band on, the class sets of
L >= 200 do not see gaps 129-1,023 (their band-off cases at 0.98 and 1.0 do),
and a pair of an L = 1,100 gap example with a short partner does not read the
long edge at all (its band-off cases do).  DESIGN.md §7.1 has the figures.

The fixtures: the six class sets, the L = 1,100 gap-field set (also each of
its edges 1,022 / 1,023 / 1,024 / 1,077 alone), the gap-power table's end
example, test_long_gap_edge's pairs, and the loop_gap 0.98 cases of the
shared-path tests.  test_old_parameters_are_blind prints (and does not
assert) what the older parameters give.
"""
import os

import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem_long_gaps as slg
from tests.helpers import make_examples

FACTOR = 100.0


def _len(o):
    return po.oracle().orc_mdata_seq_len(o.h)


def _pairs(n, limit=6):
    """Ordered pairs to try, off-diagonal first."""
    p = [(i, j) for i in range(n) for j in range(n) if i != j] + [(i, i) for i in range(n)]
    return p[:limit]


def _has(o, lo, hi):
    gaps = o.dag()["edge_gaps"]
    return bool(np.any((gaps >= lo) & (gaps <= hi)))


def _bucket_ratio(om, st, g, band, lo, hi, pairs, stop=True):
    """Best change / tolerance of su or si over the pairs that hold an edge of
    the bucket when w[lo..hi] = 0, at the case's own (loop_gap, band); stops
    at the first pair that reaches FACTOR."""
    best = 0.0
    for i, j in pairs:
        if not any(_has(o, lo, hi) for o in (om[i], om[j])):
            continue
        n = 2 * max(_len(om[i]), _len(om[j])) + 2
        for score in ("su", "si"):
            r = slg.masked_change(om[i], om[j], g, band, lo, hi, n, score) / slg.stem_tol(st[i], st[j])
            best = max(best, r)
            if stop and r >= FACTOR:
                return best
    return best


def _band_ratio(om, st, g, band, pairs):
    best = 0.0
    for i, j in pairs:
        for score in ("su", "si"):
            r = slg.band_change(om[i], om[j], g, band, score) / slg.stem_tol(st[i], st[j])
            best = max(best, r)
            if r >= FACTOR:
                return best
    return best


def _check(name, om, cases, pairs=None, blind=()):
    """Every case (loop_gap, band) as the GPU test runs it: each bucket the
    pairs hold is zeroed at that loop_gap and that band, and a case with a
    band is compared with the band off.  `blind` lists the buckets (by their
    lower end) that this fixture's cases with a band on are not asserted on:
    there the figure of the first pair is printed, and the fixture's band-off
    cases, which are asserted, are the ones that see the bucket."""
    st = [slg.dag_stats(o.dag()) for o in om]
    pairs = pairs or _pairs(len(om))
    assert max(slg.stem_tol(st[i], st[j]) for i, j in pairs) <= slg.TOL_CAP
    for g, band in cases:
        for lo, hi in slg.BUCKETS:
            if not any(_has(om[k], lo, hi) for p in pairs for k in p):
                continue
            what = f"{name} loop_gap {g} band {band}: gaps {lo}-{hi if hi < 1 << 20 else ''} zeroed"
            if band and lo in blind:
                assert any(b == 0 and h == g for h, b in cases), (name, g, "no band-off case")
                r = _bucket_ratio(om, st, g, band, lo, hi, pairs[:1], stop=False)
                print(f"{what}: change / tolerance {r:.3g} on the first pair, NOT asserted "
                      f"(seen by the band-off case at this loop_gap)")
                continue
            r = _bucket_ratio(om, st, g, band, lo, hi, pairs)
            print(f"{what}: change / tolerance {r:.3g}")
            assert r >= FACTOR, (name, g, band, lo, hi, r)
        if band:
            r = _band_ratio(om, st, g, band, pairs)
            print(f"{name} loop_gap {g}: len_band {band} against off: change / tolerance {r:.3g}")
            assert r >= FACTOR, (name, g, band, r)


# With a band on, the 129-1,023 bucket of the L >= 200 class sets stays under
# 100 tolerances (measured over all nine pairs: 2e-4 .. 0.2 at loop_gap 0.98,
# 5 .. 218 at 1.0): the cases (0.98, 0) and (1.0, 0) are the ones that see it.
CLASS_BLIND = {"L200": (129,), "L300": (129,), "L400": (129,)}


@pytest.mark.parametrize("name", list(slg.CLASS_SETS))
def test_class_sets_visible(name):
    _, om, _ = slg.built(name)
    big = slg.CLASS_SETS[name][1]
    _check(name, om, slg.PARAMS, pairs=_pairs(3, 2 if big else 6), blind=CLASS_BLIND.get(name, ()))


def test_gap_set_visible():
    """Each long edge alone, in the y role and in the x role, at every case's
    own band.  With the band off every partner reads it.  With a band on, the
    pairs of two gap examples read it (their outermost nodes are matched);
    the pairs with the L = 60 example do not (change exactly 0: no node of the
    short example is matched with the node that holds the edge): for that
    pairing the band-off cases (0.999, 0) and (1.0, 0) are the ones that count."""
    _, om, st = slg.built("gap")
    _check("gap", om, slg.GAP_PARAMS, pairs=_pairs(5, 25))
    for k, G in enumerate(slg.GAP_EDGES):
        for g, band in slg.GAP_PARAMS:
            for other in range(5):
                for i, j in ((k, other), (other, k)):
                    r = slg.masked_change(om[i], om[j], g, band, G, G, 2202) / slg.stem_tol(st[i], st[j])
                    if band and other == 4:
                        assert r == 0.0, (G, g, band, i, j, r)   # stated above; if this changes, assert it
                    else:
                        assert r >= FACTOR, (G, g, band, i, j, r)


def test_table_end_visible():
    """As tests/test_stem_long_gaps.py::test_gap_power_table_end runs it: band
    off and band 30.  The example's one stem node has length 87; under band
    10 no node of an L = 60 partner is matched with it and K is 0 in both
    roles (nothing to compare, so that band is not run); under band 30 K is 0
    with the example as x and reads the edge with the example as y."""
    seq, bpp = slg.table_end_example()
    e = po.OMData([seq], [bpp], 0.01)
    _, om60, _ = slg.built("L60")
    G = len(seq) - 4
    n = 2 * len(seq) + 2
    st_e = slg.dag_stats(e.dag())
    for o in om60:
        st = slg.dag_stats(o.dag())
        for x, y, sx, sy in ((e, o, st_e, st), (o, e, st, st_e)):
            for g in (0.98, 1.0):
                assert slg.masked_change(x, y, g, 0, G, G, n) / slg.stem_tol(sx, sy) >= FACTOR
                assert po.su_stem(x, y, g, band=10) == 0.0 and po.si_stem(x, y, g, band=10) == 0.0
        for g in (0.98, 1.0):
            assert po.su_stem(e, o, g, band=30) == 0.0
            assert slg.masked_change(o, e, g, 30, G, G, n) / slg.stem_tol(st, st_e) >= FACTOR


def test_long_gap_edge_pairs_visible():
    """tests/test_big_dag.py::test_long_gap_edge at loop_gap 0.999 and 1.0, band off (under the default band
    the pairs with a shorter partner never match the node that holds the long edge)."""
    big = np.load(os.path.join(slg.GOLDEN, "big_dag.npz"))
    s = [str(v) for v in big["seqs"]]
    om = [po.OMData([s[0]], [ska.fold(s[0].lower())], 0.01), po.OMData([s[2]], [ska.fold(s[2].lower())], 0.01),
          po.OMData([str(big["gap_seq"])], [big["gap_bpp"]], 0.01)]
    st = [slg.dag_stats(o.dag()) for o in om]
    for g in (0.999, 1.0):
        for i, j in ((2, 2), (0, 2), (2, 1)):
            tol = slg.stem_tol(st[i], st[j])
            assert tol <= slg.TOL_CAP
            r = slg.masked_change(om[i], om[j], g, 0, 1024, 1 << 30, 2202) / tol
            print(f"long-gap edge pair ({i}, {j}) loop_gap {g}: gaps >= 1,024 zeroed: change / tolerance {r:.3g}")
            assert r >= FACTOR


def _cross(n_x, n_y, limit=6):
    """Pairs (x of the first set, y of the second) of two sets laid end to end."""
    return [(i, n_x + t) for t in range(n_y) for i in range(n_x)][:limit]


def test_shared_path_twins_visible():
    """The loop_gap 0.98 cases of tests/test_gamma_shared.py, test_phi_shared.py
    and test_shared_sums.py: their inputs, each at its own band."""
    from tests.helpers import mutate_alignment
    from tests.test_gamma import _inputs
    from tests.test_gamma_shared import _path_inputs
    from tests.test_phi_shared import SEED as PHI_SEED
    from tests.test_shared_sums import _cases
    g = slg.LONG_GAP
    for name, seed in (("gamma path", 0x6A5E0), ("phi path", PHI_SEED)):
        for band in (0, 4):
            items = _path_inputs(seed + band)
            _, om = make_examples(items[:3] + items[-5:])
            _check(f"{name} band {band}", om, [(g, band)], pairs=[(0, 1), (1, 3), (3, 0), (5, 4), (4, 7), (6, 3)])
    # the row / column set twins: x of the train set, y of the test set, default band
    for name, seed in (("gamma row/column sets", 0x6A5F0), ("phi row/column sets", PHI_SEED + 0x10)):
        train = _inputs(seed)
        test = [ska.random_sequences(1, 70, seed + 1)[0], mutate_alignment(ska.random_sequences(1, 66, seed + 2)[0], 2, 3, gap=0.0)]
        _, om = make_examples(train + test)
        _check(name, om, [(g, 10)], pairs=_cross(len(train), len(test), 10))
    # test_item_queues_two_classes_long_gaps: L = 48 and L = 150, band off
    items = ska.random_sequences(14, 48, PHI_SEED + 0x20) + ska.random_sequences(3, 150, PHI_SEED + 0x21)
    _, om = make_examples(items[:3] + items[-3:])
    _check("two classes", om, [(g, 0)], pairs=[(0, 3), (3, 0), (3, 4), (5, 4), (0, 1), (4, 2)])
    for name, (items, kern, _, _) in _cases().items():
        _, om = make_examples(items[:5])
        band = kern.params.len_band
        if name == "L200":
            # band 10 and no band-off case of these four sequences: gaps 129-1,023 are printed, not asserted;
            # test_class_sets[L200-0.98-0] (sequences of the same pool and classes) is the case that sees them
            st = [slg.dag_stats(o.dag()) for o in om]
            for lo, hi in slg.BUCKETS[:2]:
                r = _bucket_ratio(om, st, g, band, lo, hi, _pairs(len(om), 4))
                print(f"shared sums L200 loop_gap {g} band {band}: gaps {lo}-{hi} zeroed: change / tolerance {r:.3g}")
                assert r >= FACTOR
            r = _bucket_ratio(om, st, g, band, 129, 1023, [(0, 1)], stop=False)
            print(f"shared sums L200 loop_gap {g} band {band}: gaps 129-1023 zeroed: change / tolerance {r:.3g}, NOT asserted")
            assert _band_ratio(om, st, g, band, [(0, 1)]) >= FACTOR
            continue
        _check("shared sums " + name, om, [(g, band)], pairs=_pairs(len(om), 4))


def test_old_parameters_are_blind():
    """Printed, not asserted: at the older tests' parameters (loop_gap 0.2,
    tolerance 1e-6) the same maskings change nothing those tests compare."""
    dag = np.load(os.path.join(slg.GOLDEN, "large_dag.npz"))
    s = [str(v) for v in dag["ns_L200_seqs"][:2]]
    om = [po.OMData([v], [ska.fold(v.lower())], 0.01) for v in s]
    for lo, hi in slg.BUCKETS[:3]:
        c = slg.masked_change(om[0], om[1], 0.2, 10, lo, hi, 402)
        print(f"ns_L200 pair (0, 1), loop_gap 0.2, band 10: gaps {lo}-{hi} zeroed: relative change {c:.3g} (tolerance 1e-6)")
    print(f"ns_L200 pair (0, 1), loop_gap 0.2: len_band 10 against off: relative change "
          f"{slg.band_change(om[0], om[1], 0.2, 10):.3g}")
    big = np.load(os.path.join(slg.GOLDEN, "big_dag.npz"))
    gap = po.OMData([str(big["gap_seq"])], [big["gap_bpp"]], 0.01)
    c = slg.masked_change(gap, gap, 0.2, 10, 1024, 1 << 30, 2202)
    print(f"test_long_gap_edge pair (gap, gap), loop_gap 0.2: gaps >= 1,024 zeroed: relative change {c:.3g}; "
          f"0.2^1077 = {0.2 ** 1077!r}")
