"""The oracle's stem_dp twins (oracle/stem_dp_generic.inc) against the pinned
double stem_dp, on the fixtures of tests/stem_long_gaps.py (CPU only):

  - the table variant with w[k] = loop_gap^k (the oracle's repeated products)
    and gap2 = loop_gap^2 is the double oracle bit for bit;
  - the long-double twin agrees with the double oracle within (D + 2) 2^-53
    relative, D the rounding depth of the pair (rounding_depth): the double
    DP's own roundings plus the twin's single rounding to double;
  - no fixture's GPU tolerance 4 D 2^-53 exceeds 1e-11;
  - the golden file holds the sets the helper module builds, and
    re-evaluating a sample of its entries reproduces them.
"""
import hashlib

import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem_long_gaps as slg

SMALL = ["L40", "L60", "L120", "gap"]
ALL = list(slg.CLASS_SETS) + ["gap"]


def _params(name):
    return slg.GAP_PARAMS if name == "gap" else slg.PARAMS


def _n_table(om_x, om_y):
    L = max(po.oracle().orc_mdata_seq_len(o.h) for o in (om_x, om_y))
    return 2 * L + 2


@pytest.mark.parametrize("name", SMALL)
def test_table_variant_is_the_double_oracle(name):
    _, om, _ = slg.built(name)
    ps, pi = ska.SuStemKernel().params, ska.SiStemKernel().params
    for g, band in _params(name) + [(0.4, 10)]:
        for a in om:
            for b in om:
                w = po.gap_weights(g, _n_table(a, b))
                assert po.su_stem_tab(a, b, w, g * g, ps.beta, band) == po.su_stem(a, b, g, ps.beta, band)
                assert po.si_stem_tab(a, b, w, g * g, pi.stack, pi.covar, band) == \
                    po.si_stem(a, b, g, pi.stack, pi.covar, band)


@pytest.mark.parametrize("name", ["L200", "L300", "L400"])
def test_table_variant_is_the_double_oracle_large(name):
    _, om, _ = slg.built(name)
    g, band = 0.98, 10
    w = po.gap_weights(g, _n_table(om[0], om[1]))
    assert po.su_stem_tab(om[0], om[1], w, g * g, 0.3, band) == po.su_stem(om[0], om[1], g, 0.3, band)
    assert po.si_stem_tab(om[1], om[0], w, g * g, 1.3, 0.8, band) == po.si_stem(om[1], om[0], g, 1.3, 0.8, band)


def test_table_variant_refuses_a_short_table():
    _, om, _ = slg.built("L40")
    assert np.isnan(po.su_stem_tab(om[0], om[1], po.gap_weights(0.98, 8), 0.98 ** 2))


@pytest.mark.parametrize("name", ALL)
def test_long_double_twin_within_rounding_depth(name):
    """Live double oracle against the reference of the GPU tests (live or
    golden): every pair at the default band, loop_gap 0.98 (0.999 for the gap
    set) and 1.0."""
    _, om, st = slg.built(name)
    ps, pi = ska.SuStemKernel().params, ska.SiStemKernel().params
    worst = 0.0
    for g, band in [p for p in _params(name) if p[1] == 10]:
        ref = slg.reference(name, g, band)
        for i, a in enumerate(om):
            for j, b in enumerate(om):
                bound = (slg.rounding_depth(st[i], st[j]) + 2) * slg.U
                for got, exp in ((po.su_stem(a, b, g, ps.beta, band), ref["su"][i, j]),
                                 (po.si_stem(a, b, g, pi.stack, pi.covar, band), ref["si"][i, j])):
                    err = abs(got - exp) / exp
                    worst = max(worst, err / bound)
                    assert err <= bound, (name, g, i, j, err, bound)
    print(f"{name}: double oracle against the long-double twin, worst error / bound {worst:.3g}")


@pytest.mark.parametrize("name", ALL)
def test_tolerance_below_cap(name):
    _, _, st = slg.built(name)
    tol = slg.tol_matrix(st)
    print(f"{name}: GPU stem tolerance {tol.min():.3g} .. {tol.max():.3g}, "
          f"classes {sorted({slg.maxk(s['nl']) for s in st})}, largest gap {max(s['gmax'] for s in st)}")
    assert tol.max() <= slg.TOL_CAP
    if name != "gap":
        assert {slg.maxk(s["nl"]) for s in st} == slg.CLASS_SETS[name][0]


def test_gap_set_edges():
    _, _, st = slg.built("gap")
    assert [s["gmax"] for s in st[:4]] == list(slg.GAP_EDGES)
    seq, bpp = slg.table_end_example()
    d = po.OMData([seq], [bpp], 0.01).dag()
    assert int(d["edge_gaps"].max()) == len(seq) - 4


@pytest.mark.parametrize("name", [n for n, (_, gold) in slg.CLASS_SETS.items() if gold])
def test_golden_inputs_are_the_helpers(name):
    z = slg.golden()
    seqs = slg.class_set(name)
    assert [str(s) for s in z[f"{name}_seqs"]] == list(seqs)
    h = hashlib.sha256()
    for s in seqs:
        h.update(np.ascontiguousarray(ska.fold(s.lower()), np.float64).tobytes())
    assert h.hexdigest() == str(z[f"{name}_sha"])
    # one entry per parameter set, re-evaluated
    _, om, _ = slg.built(name)
    for k, (g, band) in enumerate(slg.PARAMS):
        i, j = divmod(k + 1, 3)
        assert po.su_stem_ld(om[i], om[j], g, 0.3, band) == z[slg._key(name, g, band, "su")][i, j]
