"""The DAG stem kernels (dag_stem.hip, dag_stem_big.hip) where their long-gap
edges and the length band reach the compared digits: loop_gap 0.98 (0.999 at
L = 1,100) and 1.0, len_band 0 / 10 / 30, every ordered pair (the x role and
the y role differ), kinds 0, 1 and 6 (4, 5 and 7 too at L = 40 and 60; above,
their string part hides the stem part), against the long-double oracle
(oracle/stem_dp_generic.inc; live for L <= 120, tests/golden/stem_long_gaps.npz
above) at the tolerance 4 D 2^-53 of tests/stem_long_gaps.py (D: the pair's
rounding depth; at most 1e-11 on every fixture, checked on the CPU in
tests/test_stem_oracle_twin.py).  tests/test_stem_visibility_cpu.py zeroes
each gap bucket at each case's own loop_gap and band and switches the band:
the band and the gaps up to 128 move every case by 100 tolerances or more;
gaps 129-1,023 of the L >= 200 sets only the band-off cases (0.98, 0) and
(1.0, 0); a long edge of an L = 1,100 example paired with a short partner
only the band-off cases (with a band on that pair never reads it).
DESIGN.md §7.1.

  - one set of three sequences per length 40 / 60 / 120 / 200 / 300 / 400,
    picked by node count: register classes MAXK 4, 8, 12, 16, 17, 20, 24, 28
    and 32, asserted through last_classes();
  - the packed gap fields (10 bits in the y records, 16 on the x side): L =
    1,100 examples from caller bpp whose largest edge gap is 1,022, 1,023
    (saturates the y field, stays on the register-class kernel), 1,024 and
    1,077 (the big-y kernel), each in the y and in the x role, paired with
    itself, the others and an L = 60 sequence; both routes asserted;
  - the gap-power table's end: an example whose largest gap is its length - 4
    against a set of shorter examples, through test_matrix and test_row in
    both set orders (a table sized from the wrong set is read past its end).

Measured GPU error (max over a family of |got - ref| / ref for the stem
kinds, and of error / tolerance): see MEASURED below.
"""
import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem_long_gaps as slg

pytestmark = pytest.mark.gpu

# From a run on an MI355X (pytest -s prints the figures per test): family ->
# (max relative error of kinds 0 and 1, max error / tolerance).
MEASURED = {
    "class sets L40 .. L400, every (loop_gap, band)": (2.1e-15, 1.3e-3),
    "gap fields 1,022 / 1,023 / 1,024 / 1,077": (1.5e-15, 5.8e-3),
    "gap-power table's end": (2.2e-16, 1.3e-3),
}


def _all_pairs(n):
    x, y = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    return x, y


def _run_kinds(ctx, ds, name, g, band, tol, x=None, y=None, kinds=slg.KINDS):
    """Every kind on the pairs (x, y) (default: all ordered pairs) of a set
    with a stored reference; returns the classes that ran (union)."""
    ref = slg.reference(name, g, band)
    n = len(ds)
    full = x is None
    if full:
        x, y = _all_pairs(n)
    sub = {k: v[x, y] for k, v in ref.items()}
    ran = set()
    for kind in kinds:
        kern = slg.kernel(kind, g, band)
        got = ctx.pairs(ds, kern, x, y)
        ran |= set(ctx.last_classes()["stem_maxk"])
        worst, rel = slg.excess(kind, got, sub, tol[x, y], kern.params)
        print(f"{name} loop_gap {g} band {band} kind {kind}: max rel err {rel:.3g}, err / allowed {worst:.3g}")
        assert worst <= 1.0, (name, g, band, kind, worst)
    return ran


@pytest.mark.parametrize("g,band", slg.PARAMS)
@pytest.mark.parametrize("name", list(slg.CLASS_SETS))
def test_class_sets(gpu_ctx, name, g, band):
    ds, _, st = slg.built(name)
    tol = slg.tol_matrix(st)
    assert tol.max() <= slg.TOL_CAP
    # kinds 4, 5 and 7 on the two short sets only: they allow STR_TOL * K_str, which outweighs the whole stem part
    # from L ~ 60 up (K_str is 1e88-1e91 at L = 400), so they check the composition, not the stem
    kinds = slg.KINDS if name in ("L40", "L60") else slg.STEM_KINDS
    ran = _run_kinds(gpu_ctx, ds, name, g, band, tol, kinds=kinds)
    print(f"{name}: classes {sorted(ran)}, tolerance {tol.min():.3g} .. {tol.max():.3g}")
    assert slg.CLASS_SETS[name][0] <= ran, ran
    assert 0 not in ran


@pytest.mark.parametrize("g,band", slg.GAP_PARAMS)
def test_gap_fields(gpu_ctx, g, band):
    """Examples 0..3: largest edge gap 1,022 / 1,023 / 1,024 / 1,077; 4: L = 60.
    Kinds 0, 1 and 6: the string part of 4, 5 and 7 overflows double at L = 1,100."""
    ds, _, st = slg.built("gap")
    tol = slg.tol_matrix(st)
    assert [s["gmax"] for s in st[:4]] == list(slg.GAP_EDGES)
    allx = np.arange(5, dtype=np.int32)
    for yk in range(5):  # one y per call: the route of that y
        ran = _run_kinds(gpu_ctx, ds, "gap", g, band, tol, allx, np.full(5, yk, np.int32), kinds=slg.STEM_KINDS)
        print(f"y example {yk} (largest gap {st[yk]['gmax']}): classes {sorted(ran)}")
        if st[yk]["gmax"] > 1023:
            assert ran == {0}, (yk, ran)        # the big-y kernel alone
        else:
            assert ran and 0 not in ran, (yk, ran)  # 1,023 still fits the 10-bit field; x gaps have 16 bits
    ran = _run_kinds(gpu_ctx, ds, "gap", g, band, tol, kinds=slg.STEM_KINDS)   # all 25 pairs in one call: both kernels
    assert 0 in ran and any(k > 0 for k in ran), ran


def test_gap_power_table_end(gpu_ctx):
    seq, bpp = slg.table_end_example()
    e_ds, e_om = slg.build([(seq, bpp)])
    assert int(e_ds.dag(0)["edge_gaps"].max()) == len(seq) - 4
    s_ds, s_om, s_st = slg.built("L60")
    e_st = [slg.dag_stats(e_om[0].dag())]
    ps, pi = ska.SuStemKernel().params, ska.SiStemKernel().params
    # band 10 is left out: K is 0 for every pair of this example with a shorter one, in both roles; under band
    # 30 it is 0 with the example as x and reads the long edge with it as y (tests/test_stem_visibility_cpu.py)
    for g, band in ((0.98, 0), (1.0, 0), (0.98, 30), (1.0, 30)):
        for kind in (0, 1):
            kern = slg.kernel(kind, g, band)
            ld = (lambda a, b: po.su_stem_ld(a, b, g, ps.beta, band)) if kind == 0 else \
                (lambda a, b: po.si_stem_ld(a, b, g, pi.stack, pi.covar, band))
            # the long example in the y role: K(short[j], long)
            ref_y = np.array([ld(o, e_om[0]) for o in s_om])
            tol_y = slg.tol_matrix(s_st, e_st)[:, 0]
            # ... and in the x role: K(long, short[i])
            ref_x = np.array([ld(e_om[0], o) for o in s_om])
            tol_x = slg.tol_matrix(e_st, s_st)[0]
            m_y, _ = gpu_ctx.test_matrix(e_ds, s_ds, kern)       # out[0, j] = K(short[j], long)
            m_x, _ = gpu_ctx.test_matrix(s_ds, e_ds, kern)       # out[i, 0] = K(long, short[i])
            r_y = gpu_ctx.test_row(e_ds, 0, s_ds, kern)          # out[j] = K(short[j], long)
            r_x = np.array([gpu_ctx.test_row(s_ds, i, e_ds, kern)[0] for i in range(len(s_ds))])
            for what, got, ref, tol in (("matrix, long y", m_y[0], ref_y, tol_y), ("matrix, long x", m_x[:, 0], ref_x, tol_x),
                                        ("row, long y", r_y, ref_y, tol_y), ("row, long x", r_x, ref_x, tol_x)):
                err = np.abs(got - ref)
                rel = np.max(err / np.where(ref > 0, ref, 1.0))
                print(f"table end, loop_gap {g} band {band} kind {kind}, {what}: max rel err {rel:.3g}, "
                      f"err / tolerance {np.max(err / np.where(ref > 0, tol * ref, 1.0)):.3g}")
                assert np.all(err <= tol * ref), (g, band, kind, what)
                if band == 0 or what.endswith("long y"):
                    assert np.all(ref > 0)
