"""The oracle's string DP twins (oracle/sk_oracle.c: orc_profile_string_ld,
orc_naive_string_ld, orc_profile_string_tab, orc_naive_string_tab) against
the pinned double DPs, on the fixtures of tests/string_long_gaps.py (CPU):

  - the long-double twin agrees with the double oracle within D 2^-53
    relative (D: rounding_depth of the pair at the oracle's own factor
    roundings), a quarter of the GPU tolerance 4 D 2^-53 by construction; the
    measured fraction of the GPU tolerance is printed and bounded;
  - the table twin with geometric long-double tables is the _ld twin to one
    ulp of double;
  - no fixture's GPU tolerance exceeds 1e-11;
  - where the reference's own DP code is built, it and the twins agree on
    the pinning suite's small inputs.
"""
import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem_long_gaps as slg
from tests import string_long_gaps as sg
from tests.helpers import make_examples, mutate_alignment

# the double oracle's factor roundings are the general kernel's (3), 1 in the naive mode
ORACLE_PATH = "general"


def _fraction(dbl, ld, tol):
    assert np.all(np.isfinite(ld))
    return float(np.max(np.abs(dbl - ld) / (tol * ld)))


@pytest.mark.parametrize("variant,use_bp", [(v, bp) for v in sg.VARIANTS for bp in (False, True)
                                            if not (v == "mixed" and not bp)])
def test_long_double_twin_on_probes(variant, use_bp):
    _, om, first, lens, _ = sg.probe_set(variant, use_bp)
    naive = sg.VARIANTS[variant][5]
    tol = sg.tol_matrix(lens, path="naive" if naive else ORACLE_PATH)
    assert tol.max() <= sg.TOL_CAP
    n = len(om)
    for g in (0.98, 1.0):
        ld = sg.probe_reference(variant, use_bp, g)
        if naive:
            dbl = np.array([[po.naive_string(first[a], first[b], g) for b in range(n)] for a in range(n)])
        else:
            dbl = np.array([[po.si_str(om[a], om[b], g, 1.0, 0.0) for b in range(n)] for a in range(n)])
        fr = _fraction(dbl, ld, tol)
        print(f"probes {variant} use_bp {use_bp} gap {g}: double oracle - twin, worst / GPU tolerance {fr:.3g}")
        assert fr <= 0.25


@pytest.mark.parametrize("name", sg.DENSE_SETS)
def test_long_double_twin_on_dense_sets(name):
    _, om, lens, _ = sg.dense_set(name)
    tol = sg.tol_matrix(lens, path=ORACLE_PATH)
    assert sg.tol_matrix(lens).max() <= sg.TOL_CAP
    for which in sg.DENSE_KERNELS:
        for g in sg.DENSE_GAPS:
            ld = sg.dense_reference(name, which, g)
            p = sg.dense_kernel(which, g).params
            dbl = np.array([[po.kernel_value(p.kind, a, b, p) for b in om] for a in om])
            fr = _fraction(dbl, ld, tol)
            print(f"dense {name} {which} gap {g}: double oracle - twin, worst / GPU tolerance {fr:.3g}, "
                  f"K up to {ld.max():.3g}")
            assert fr <= 0.25


def test_table_twin_is_the_long_double_twin():
    """Geometric tables: the same DP, summed in another order."""
    worst = 0.0
    for variant in ("aln3", "naive"):
        _, om, first, lens, _ = sg.probe_set(variant, True)
        naive = sg.VARIANTS[variant][5]
        for g in (0.98, 1.0):
            ld = sg.probe_reference(variant, True, g)
            for a in range(0, len(om), 5):
                for b in range(sg.N_X + a % 2, len(om), 7):
                    tab = po.string_tables(g, lens[a], lens[b])
                    t = po.naive_string_tab(first[a], first[b], g, tab) if naive else \
                        po.si_str_tab(om[a], om[b], tab, 1.0, 0.0)
                    worst = max(worst, abs(t - ld[a, b]) / ld[a, b])
    _, om, lens, _ = sg.dense_set("single")
    for g in sg.DENSE_GAPS:
        for a, b in ((0, 5), (20, 9), (22, 11), (10, 21), (12, 13)):
            tab = po.string_tables(g, lens[a], lens[b])
            for t, ld in ((po.su_str_tab(om[a], om[b], tab, sg.ALPHA), sg.dense_reference("single", "su", g)[a, b]),
                          (po.si_str_tab(om[a], om[b], tab, sg.MATCH, sg.MISMATCH),
                           sg.dense_reference("single", "si", g)[a, b])):
                worst = max(worst, abs(t - ld) / ld)
    print(f"table twin against the _ld twin: worst relative difference {worst:.3g} ({worst / sg.U:.2f} x 2^-53)")
    assert worst <= 2 * sg.U


def test_table_twin_refuses_a_short_table():
    _, om, _, lens, _ = sg.probe_set("onehot", False)
    tab = po.string_tables(0.98, lens[0], lens[-1] - 1)
    with pytest.raises(ValueError):
        po.si_str_tab(om[0], om[-1], tab, 1.0, 0.0)


def test_sum_kind_tolerances_below_cap():
    for name in slg.CLASS_SETS:
        _, om, st = slg.built(name)
        lens = [po.oracle().orc_mdata_seq_len(o.h) for o in om]
        t = sg.tol_matrix(lens, path="onehot")
        print(f"{name}: string tolerance {t.max():.3g}, stem tolerance {slg.tol_matrix(st).max():.3g}")
        assert t.max() <= sg.TOL_CAP
        k2, k3 = sg.sum_string_reference(name)
        assert np.all(np.isfinite(k2)) and np.all(np.isfinite(k3))


def test_twins_against_the_reference_dp():
    """The reference's own string DPs (oracle/_ref) on the pinning suite's
    kind of inputs: short sequences and alignments, every ordered pair."""
    if not po.reference_dp_expected():
        pytest.skip("no reference build")
    seqs = ska.random_sequences(4, 30, 0x5EED0C00) + ["ACGUNRYKMSWACGU", "GGGAAACCC"]
    alns = [mutate_alignment(seqs[0], 3, 3), mutate_alignment(seqs[1][:20], 2, 4, gap=0.0)]
    _, om = make_examples(seqs + alns)
    bpps = [[ska.fold(r.replace("-", "").lower()) for r in ([e] if isinstance(e, str) else e)] for e in seqs + alns]
    rm = [po.RMData([e] if isinstance(e, str) else e, b) for e, b in zip(seqs + alns, bpps)]
    for kern in (ska.StringKernel(gap=0.8, alpha=0.2), ska.StringKernel(gap=0.98, match=1.0, mismatch=0.6)):
        p = kern.params
        for a in range(len(om)):
            for b in range(len(om)):
                ref = po.ref_kernel_value(p.kind, rm[a], rm[b], p)
                la, lb = (po.oracle().orc_mdata_seq_len(o.h) for o in (om[a], om[b]))
                ld = po.su_str_ld(om[a], om[b], p.gap, p.alpha) if p.kind == 2 else \
                    po.si_str_ld(om[a], om[b], p.gap, p.match, p.mismatch)
                tab = po.string_tables(p.gap, la, lb)
                tb = po.su_str_tab(om[a], om[b], tab, p.alpha) if p.kind == 2 else \
                    po.si_str_tab(om[a], om[b], tab, p.match, p.mismatch)
                bound = sg.rounding_depth(la, lb, ORACLE_PATH) * sg.U
                assert abs(ref - ld) <= bound * ld and abs(tb - ld) <= 2 * sg.U * ld, (a, b, ref, ld, tb)
    for g in (0.8, 0.98, 1.0):
        for x in seqs:
            for y in seqs:
                ref, ld = po.ref_naive_string(x, y, g), po.naive_string_ld(x, y, g)
                tb = po.naive_string_tab(x, y, g, po.string_tables(g, len(x), len(y)))
                assert abs(ref - ld) <= sg.rounding_depth(len(x), len(y), "naive") * sg.U * ld
                assert abs(tb - ld) <= 2 * sg.U * ld
