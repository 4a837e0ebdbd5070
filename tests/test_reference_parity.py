"""The HIP kernels against the reference's own DP code, directly.

The other GPU tests compare with the oracle (oracle/sk_oracle.c), which
tests/test_oracle_dp_pinning.py pins to the reference on the CPU.  Here the
kernels meet the reference itself (oracle/_ref/libskref_{lite,4d,str,bpla}.so:
its DP sources compiled in place by oracle/Makefile) with no restatement in
between: every lite kind over all ordered pairs of six examples, full_dp,
banded and PairHMM-constrained 4-D pairs, the naive string kernel, and BPLA
values and gradients.  1e-6 relative, the project's GPU tolerance.  Only the
built libraries are read; the reference tree is not needed to run this."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import refdp
from tests.helpers import make_examples

pytestmark = pytest.mark.gpu

if not refdp.need_reference_dp():
    pytest.skip("neither the reference tree nor oracle/_ref is present", allow_module_level=True)

TOL = 1e-6


def _lite_items():
    """Six examples of L 20-60 cut from the CPU pinning set: two single
    sequences, a gapless 3-row and a gapped 2-row and 3-row alignment, IUPAC."""
    it = refdp.lite_items()
    return [it[0][:56], [r[:60] for r in it[1]], [r[:48] for r in it[2]], it[5], it[6], it[7]]


@pytest.fixture(scope="module")
def lite_set():
    items = _lite_items()
    assert len(items) == 6 and all(20 <= len(refdp.rows_of(ex)[0]) <= 60 for ex in items)
    ds, _ = make_examples(items)
    rm = []
    for ex in items:
        rows = refdp.rows_of(ex)
        rm.append(po.RMData(rows, refdp.fold_rows(rows), 0.01))
    return ds, rm


@pytest.mark.parametrize("kind", list(refdp.LITE_KINDS))
def test_lite_kind_matches_reference(gpu_ctx, lite_set, kind):
    ds, rm = lite_set
    n = len(rm)
    kern = refdp.lite_kernel(kind, band=4)
    x, y = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    got = gpu_ctx.pairs(ds, kern, x, y)
    ref = [po.ref_kernel_value(kind, rm[i], rm[j], kern.params) for i, j in zip(x, y)]
    w = refdp.worst_rel(got, ref)
    print(f"kind {kind}: worst rel {w:.3g}")
    assert np.all(np.isfinite(ref)) and w < TOL


@pytest.mark.parametrize("cfg", ["full_dp", "band", "phmm"])
def test_stem4d_matches_reference(gpu_ctx, cfg):
    """full_dp, partial_dp with a -b band, and partial_dp under the PairHMM
    constraints as the reference computes them when built today
    (ali_zerop_fixed = 0), at L 24, both orders of one pair."""
    kw = {"full_dp": {}, "band": dict(band=3), "phmm": dict(ali_bound=0.5, band=2)}[cfg]
    seqs = refdp.stem4d_seqs()[:2]
    assert all(len(s) == 24 for s in seqs)
    ds, _ = make_examples(seqs)
    kern = ska.StemKernel4D(gap=0.75, stack=1.25, subst=0.5, ali_zerop_fixed=False, **kw)
    p = kern.params
    got = gpu_ctx.pairs(ds, kern, [0, 1], [1, 0])
    ref = [po.ref_stem4d(seqs[a].lower(), ska.fold(seqs[a]), seqs[b].lower(), ska.fold(seqs[b]),
                         p.gap, p.stack, p.subst, p.bp_bound, p.bp_model, p.loop, p.len_band,
                         p.ali_bound) for a, b in ((0, 1), (1, 0))]
    w = refdp.worst_rel(got, ref)
    print(f"4-D {cfg}: worst rel {w:.3g}, K = {ref}")
    assert min(ref) > 1.0 and w < TOL


def test_naive_string_matches_reference(gpu_ctx):
    strs = ska.random_sequences(2, 40, 77) + ["AC", "A"]
    ds, _ = make_examples(strs, use_bp=False)
    n = len(strs)
    x, y = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    got = gpu_ctx.pairs(ds, ska.NaiveStringKernel(gap=0.7), x, y)
    ref = [po.ref_naive_string(strs[i], strs[j], 0.7) for i, j in zip(x, y)]
    assert refdp.worst_rel(got, ref) < TOL


@pytest.fixture(scope="module")
def bpla_set():
    alns = refdp.bpla_alignments()[:4]
    assert all(len(a[0]) <= 45 for a in alns)
    ds, _ = make_examples(alns)
    rb = [po.RBData(rows, refdp.fold_rows(rows)) for rows in alns]
    n = len(alns)
    x, y = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    return ds, rb, x, y


@pytest.mark.parametrize("sw", [False, True])
@pytest.mark.parametrize("no_bp", [False, True])
def test_bpla_values_match_reference(gpu_ctx, bpla_set, no_bp, sw):
    ds, rb, x, y = bpla_set
    kern = ska.BPLAKernel(noBP=no_bp, SW=sw, alpha=2.0, beta=0.2)
    p = kern.params
    got = gpu_ctx.pairs(ds, kern, x, y)
    ref = [po.ref_bpla(rb[i], rb[j], no_bp, sw, p.gap, p.ext, p.alpha, p.beta, list(p.score_table))
           for i, j in zip(x, y)]
    w = refdp.worst_rel(got, ref)
    print(f"BPLA no_bp={no_bp} sw={sw}: worst rel {w:.3g}")
    assert w < TOL


def test_bpla_gradients_match_reference(gpu_ctx, bpla_set):
    ds, rb, x, y = bpla_set
    kern = ska.BPLAKernel(alpha=2.0, beta=0.2)
    p = kern.params
    t = np.array(list(p.score_table))
    val, grad = gpu_ctx.bpla_gradients(ds, kern, x, y)
    rv, rg = [], []
    for i, j in zip(x, y):
        v, d = po.ref_bpla_gradients(rb[i], rb[j], p.alpha, p.beta, p.gap, p.ext, t)
        rv.append(v)
        rg.append(d)
    rg = np.array(rg)
    worst = [refdp.worst_rel(val, rv)] + [refdp.worst_rel(grad[:, k], rg[:, k]) for k in range(4)]
    print("BPLA worst rel (value, d_alpha, d_beta, d_gap, d_ext):", worst)
    assert np.all(rg != 0.0) and max(worst) < TOL
