"""The long-double twin of the oracle's 4-D DPs (oracle/stem4d_generic.inc):
its double instantiation is po.stem4d bit for bit, the long-double one agrees
with it within the derived rounding bound, and the probes' closed form equals
the twin on every family scaled down to the twin's cost.  DESIGN.md §7.3."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem4d_probes as sp


def _bit_seqs():
    return ska.random_sequences(2, 24, 0x5EED0091) + ska.random_sequences(1, 17, 0x5EED0092) + \
        ska.random_sequences(1, 41, 0x5EED0093) + ["", "G", "GGGAAACCC"]


@pytest.mark.parametrize("band", [0, 1, 3, 8, 100])
@pytest.mark.parametrize("model,bound", [(0, 0.0), (0, 0.2), (1, 0.5), (2, 0.5)])
def test_double_instance_is_oracle_bit_for_bit(band, model, bound):
    """Every pair in both orders (asymmetric lengths 17 / 24 / 41, the empty
    and a one-residue sequence), full_dp and -b bands, the three bp models."""
    seqs = _bit_seqs()
    for a in seqs:
        for b in seqs:
            bx = ska.fold(a) if a else np.zeros(0)
            by = ska.fold(b) if b else np.zeros(0)
            args = (a.lower(), bx if model == 0 else None, b.lower(), by if model == 0 else None,
                    sp.f32(0.8), 1.3, 0.4, bound, model, 3, band)
            assert po.stem4d_gen(*args) == po.stem4d(*args), (a, b)


@pytest.mark.parametrize("gap", sp.DENSE_GAPS)
@pytest.mark.parametrize("band", [0, 3, 100])
def test_twin_agrees_with_oracle(gap, band):
    """Within 4 D 2^-53: the oracle sums along the K chain, so the source
    count S of the kernels' other summation orders does not enter."""
    seqs = _bit_seqs() + ska.random_sequences(1, 70, 0x5EED0013)
    worst = 0.0
    for a in seqs:
        for b in seqs[:5] + seqs[-1:]:
            bx = ska.fold(a) if a else np.zeros(0)
            by = ska.fold(b) if b else np.zeros(0)
            args = (a.lower(), bx, b.lower(), by, sp.f32(gap), 1.0, 0.5, 0.0, 0, 3, band)
            dbl, ld = po.stem4d(*args), po.stem4d_ld(*args)
            t = sp.tol(len(a), len(b), 0, 0, band > 0)
            worst = max(worst, abs(dbl - ld) / ld / t)
            assert abs(dbl - ld) <= t * ld, (a, b, dbl, ld, t)
    print(f"gap {gap} band {band}: oracle against twin, largest error / tolerance {worst:.3g}")


@pytest.mark.parametrize("family", sp.FAMILIES)
def test_closed_form_equals_twin(family):
    """Every probe of the family scaled down to sequences <= 140, at its
    first gap and at 0.8, every fourth also at 1.0; full_dp, and a band wider
    than both sequences for every eighth (partial_dp computes every cell)."""
    worst = 0.0
    for n, pr in enumerate(sp.probes(family, small=True)):
        gaps = [sp.probe_gaps(pr)[0], sp.DEFAULT_GAP] + ([1.0] if n % 4 == 0 else [])
        for g in gaps:
            cf = float(sp.closed_form(pr, g))
            for band in (0, 200) if n % 8 == 0 else (0,):
                tw = sp.twin_of_probe(pr, g, band=band)
                t = sp.probe_tol(pr, band > 0)
                worst = max(worst, abs(tw - cf) / cf / t)
                assert abs(tw - cf) <= t * cf, (pr.name, g, band, tw, cf)
    print(f"{family}: twin against closed form, largest error / tolerance {worst:.3g}")


def test_closed_form_two_pair_example():
    """K = 1 + outer + inner + nested on a two-pair example, term by term."""
    pr = sp.probes("nested")[0]
    assert pr.name == "ne_k0_m140" and pr.xp == ((0, 11, 0.75), (1, 10, 0.5))
    for g in (sp.f32(0.8), sp.f32(0.98), 1.0):
        po_, pi_, qo, qi = 0.75, 0.5, 0.75, 0.5
        m = 140
        # sources (x pair, y pair) and the G0 each reads; only (outer, outer) holds a nesting
        k = 1 + po_ * qo * (g ** (10 + m - 2) + g ** (8 + m - 4)) + 0.5 * po_ * qi * g ** (10 + m - 4) \
            + 0.5 * pi_ * qo * g ** (8 + m - 2) + pi_ * qi * g ** (8 + m - 4)
        assert abs(float(sp.closed_form(pr, g)) - k) <= 1e-14 * k
        assert abs(po.stem4d(pr.x.lower(), sp.packed_bpp(12, pr.xp), pr.y.lower(), sp.packed_bpp(m, pr.yp), g) - k) \
            <= 1e-13 * k
