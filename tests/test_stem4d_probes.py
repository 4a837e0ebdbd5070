"""The 4-D stem kernels (stem4d.hip: column-group, pre-combined span, K-sum
span with k tiles, four-state partial_dp) where long unpaired runs, table
ends and tile seams reach the compared digits: sparse probes against their
closed form and dense sets against the long-double twin, both within the
tolerance derived from the DP's roundings (tests/stem4d_probes.py, DESIGN.md
§7.3), at gap 0.98 / 0.999 / 1.0 and once at the default 0.8.  Every test
asserts the kernel that ran and prints its largest relative error beside the
tolerance."""
import hashlib

import numpy as np
import pytest

import stem_kernel_amd as ska
from stem_kernel_amd.kernel_matrix import stem4d_col_shape
from tests import stem4d_probes as sp

WIDE = 4096   # a band wider than every sequence here: partial_dp computes every cell


def _cpl(m):
    return 1 if m + 1 <= 64 else 2 if m + 1 <= 128 else 4 if m + 1 <= 256 else 8


def _expected(prs, banded, variant=None):
    """(last_classes()["stem4d"], ["stem4d_col"]) of a call over the probes:
    the class follows the call's longest y; |y| >= 512 runs k tiles, |x| >
    2,048 and the variants the span kernels, -b the four-state kernel, the
    rest the column kernel."""
    m, n = max(len(p.y) for p in prs), max(len(p.x) for p in prs)
    c = _cpl(m)
    col = not banded and variant is None and m < 512 and n <= 2048
    return [(c, banded)], [c] if col else []


def _run(gpu_ctx, prs, key, gaps, bands, variant=None):
    ds, xi, yi = sp.probe_dataset(prs)
    out = []
    for g in gaps:
        ref = np.array([sp.probe_ref(key + (p.name,), g) for p in prs])
        for band in bands:
            kern = ska.StemKernel4D(gap=g, band=band)
            assert kern.params.gap == g and kern.params.bp_bound == 0.0
            got = gpu_ctx.pairs(ds, kern, xi, yi)
            cls = gpu_ctx.last_classes()
            assert (cls["stem4d"], cls["stem4d_col"]) == _expected(prs, band > 0, variant), (g, band, cls)
            tols = np.array([sp.probe_tol(p, band > 0) for p in prs])
            worst, rel, top = sp.excess(got, ref, tols)
            out.append((g, band, worst, rel, top))
            print(f"{prs[0].family}/{prs[0].group} gap {g:.6g} band {band}: {len(prs)} probes, largest relative "
                  f"error {rel:.3g}, tolerance {top:.3g}")
    for g, band, worst, rel, top in out:
        assert worst <= 1.0, (prs[0].group, g, band, rel, top)


def _group_params():
    return [(f, g) for f in sp.FAMILIES for g in sp.groups(f)]


@pytest.mark.gpu
@pytest.mark.parametrize("family,group", _group_params())
def test_probe_group_matches_closed_form(gpu_ctx, family, group):
    """One probe group (one y length class, one pairs() call per gap and
    mode): full_dp on the kernel its lengths select, and the same probes
    under a band wider than both sequences through the four-state kernel,
    against the same closed form; at the probes' gaps and at the default 0.8.
    For |x| > 2,000 the wide band runs at gap 0.999 only: a four-state call
    of 2,049 x 40 takes 1-2 s, and at 0.999 a dropped term and a shifted
    gap-power index both show (at 1.0 every power is 1, at 0.8 the term is
    below the tolerance), so the other two gaps would add time and nothing
    that 0.999 does not see."""
    prs = sp.groups(family)[group]
    gaps = sorted({g for p in prs for g in sp.probe_gaps(p)} | {sp.DEFAULT_GAP})
    if family == "nested":
        # W from the batch's shortest y: 8 for the k / l sweeps, m - 3 = 5 for the i / j sweeps' short y
        m = {len(p.y) for p in prs}
        assert len(m) == 1
        assert stem4d_col_shape(min(m), max(m))["waves"] == (5 if group == f"y{sp.NESTED_SHORT_Y}" else 8)
    if max(len(p.x) for p in prs) > 2000:
        _run(gpu_ctx, prs, (family, False), gaps, (0,))
        _run(gpu_ctx, prs, (family, False), (sp.f32(0.999),), (WIDE,))
    else:
        _run(gpu_ctx, prs, (family, False), gaps, (0, WIDE))


@pytest.mark.gpu
@pytest.mark.explib
@pytest.mark.parametrize("variant", ["pre", "ksum", "four"])
def test_probe_variants_match_closed_form(gpu_ctx, monkeypatch, variant):
    """The kernels the default call does not pick, on the probes of the
    column kernel's range: the pre-combined span kernel (SK4_SPAN), the K-sum
    span kernel (SK4_NO_PRE) and full_dp on the four-state planes
    (SK4_NO_GSUM).  last_classes() reports the span launches' CPL and whether
    they were banded, not which span kernel ran: what is asserted here is
    that the column kernel did not run (stem4d_col == []) and the class; that
    each switch selects the kernel it names is the planner's code
    (host/pairs_stem4d.cpp: gsum, colk_call, no_pre)."""
    monkeypatch.setenv({"pre": "SK4_SPAN", "ksum": "SK4_NO_PRE", "four": "SK4_NO_GSUM"}[variant], "1")
    for family, group in (("nested", "m140"), ("nested", "m60"), ("nested", f"y{sp.NESTED_SHORT_Y}"),
                          ("table_end", "m128"), ("table_end", "m511"), ("long_x", "n700")):
        prs = sp.groups(family)[group]
        gaps = sorted({g for p in prs for g in sp.probe_gaps(p)})
        _run(gpu_ctx, prs, (family, False), gaps, (0,), variant)


def _dense_params():
    return [(n, g, b) for n in sp.DENSE_SETS for g in sp.DENSE_GAPS for b in sp.DENSE_BANDS]


def test_golden_fold_bytes_pinned():
    h = hashlib.sha256()
    for name in sp.DENSE_SETS + ("col", "tiled"):
        for s in sp.dense_set(name)[0]:
            h.update(np.ascontiguousarray(sp.folded(s), np.float64).tobytes())
    assert h.hexdigest() == str(sp.golden()["sha"])


def _dense(gpu_ctx, name, gap, band):
    seqs, pairs = sp.dense_set(name)
    ds = ska.Dataset.from_sequences(list(seqs), bpp=[sp.folded(s) for s in seqs])
    kern = ska.StemKernel4D(gap=gap, band=band)
    got = gpu_ctx.pairs(ds, kern, [a for a, _ in pairs], [b for _, b in pairs])
    cls = gpu_ctx.last_classes()
    tols = sp.pair_tols(seqs, pairs, kern.params)
    worst, rel, top = sp.excess(got, sp.dense_ref(name, gap, band), tols)
    print(f"{name} gap {gap} band {band}: {len(pairs)} pairs, largest relative error {rel:.3g}, "
          f"tolerance {top:.3g}, error / tolerance {worst:.3g}")
    return cls, worst, max(len(seqs[b]) for _, b in pairs)


@pytest.mark.gpu
@pytest.mark.parametrize("name,gap,band", _dense_params())
def test_dense_set_matches_twin(gpu_ctx, name, gap, band):
    """The suite's Gram, the two L = 130 sequences and the lopsided 24 x 300 /
    457 pairs at gap 0.8, 0.98 and 1.0, full_dp (the column kernel) and -b 1,
    3, 8 (the four-state kernel), against the twin's golden values."""
    cls, worst, m = _dense(gpu_ctx, name, gap, band)
    c = _cpl(m)
    assert cls["stem4d"] == [(c, band > 0)] and cls["stem4d_col"] == ([] if band else [c]), cls
    assert worst <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("gap", sp.DENSE_GAPS)
def test_banded_pair_over_k_tiles_matches_twin(gpu_ctx, gap):
    """24 x 1,040 under -b 100: the four-state kernel over three k tiles, the
    band's windows holding the seam k = 512 for four values of i
    (tests/test_stem4d_visibility_cpu.py asserts that from the oracle's band)."""
    cls, worst, _ = _dense(gpu_ctx, "tiled", gap, sp.TILED_BAND)
    assert cls["stem4d"] == [(8, True)] and not cls["stem4d_col"], cls
    assert worst <= 1.0
