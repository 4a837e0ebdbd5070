"""Pin the oracle's DPs to the reference's own DP code.

oracle/_ref/libskref_{lite,4d,str,bpla}.so are the reference's DP translation
units -- the DAG builder and every kernel of stem_kernel_lite, the 4-D stem
kernel with its PairHMM, the naive string kernel and the BPLA kernel with its
gradients -- compiled unmodified and in place by oracle/Makefile against the
project's stand-in headers for the few Boost names they use.  Base-pairing
probabilities enter at the BPMatrix seam (oracle/ref_shim/bpmatrix_seam.hpp);
the averaging of per-row matrices into an alignment's matrix and ViennaRNA's
folding are the parts that stay unpinned.

Tolerance: the oracle claims the reference's operation order and both are
built with contraction off, so the expected difference is zero.  The worst
relative difference measured per family on these inputs is 0 (bit equality,
DESIGN.md §7 table); the bound is ten times that with a floor of 1e-15.
Each test prints its worst figure before asserting."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import refdp

if not refdp.need_reference_dp():
    pytest.skip("neither the reference tree nor oracle/_ref is present", allow_module_level=True)

TOL = 1e-15  # max(10 x measured worst (0), 1e-15); never above 1e-12


# ------------------------------------------------------------------ lite: examples
@pytest.mark.parametrize("th", [0.01, 0.05])
def test_built_examples_match_reference(th):
    """Profiler, DAGBuilder, find_root, find_max_parent and fill_weight: nodes,
    edges with gaps, bp-frequency entries, roots, max_pa and weights."""
    om, rm = refdp.lite_examples(th)
    n_nodes = []
    for ex, o, r in zip(refdp.lite_items(), om, rm):
        do, dr = o.dag(), r.dag()
        assert do.keys() == dr.keys()
        for k in do:
            assert np.array_equal(do[k], dr[k]), (ex, k)
        n_nodes.append(len(dr["first"]))
    print("nodes per example:", n_nodes)
    assert n_nodes[-1] == 0 and min(n_nodes[:-1]) > 0  # the empty DAG is in the set


# ------------------------------------------------------------------ lite: kernels
@pytest.mark.parametrize("band", [0, 1, 4])
@pytest.mark.parametrize("th", [0.01, 0.05])
def test_lite_kernels_match_reference(th, band):
    """All eight kinds on every ordered pair (the stem kernels are not
    symmetric in their evaluation order), non-default parameters."""
    om, rm = refdp.lite_examples(th)
    n = len(om)
    worst = {}
    for kind in refdp.LITE_KINDS:
        p = refdp.lite_kernel(kind, band).params
        assert p.kind == kind
        o = [[po.kernel_value(kind, om[i], om[j], p) for j in range(n)] for i in range(n)]
        r = [[po.ref_kernel_value(kind, rm[i], rm[j], p) for j in range(n)] for i in range(n)]
        worst[kind] = refdp.worst_rel(o, r)
        if kind == 0:
            assert np.count_nonzero(np.asarray(r)) > n  # the band leaves pairs to compare
    print(f"th={th} band={band} worst rel per kind:", worst)
    assert max(worst.values()) <= TOL, worst


def test_lite_string_kernels_without_weights_match_reference():
    """MData(ma): no base-pair information, the unweighted branch."""
    om, rm = refdp.lite_examples(0.01, use_bp=False)
    n = len(om)
    worst = {}
    for kind in (2, 3):
        p = refdp.lite_kernel(kind, 0).params
        o = [[po.kernel_value(kind, om[i], om[j], p) for j in range(n)] for i in range(n)]
        r = [[po.ref_kernel_value(kind, rm[i], rm[j], p) for j in range(n)] for i in range(n)]
        worst[kind] = refdp.worst_rel(o, r)
    print("worst rel per kind:", worst)
    assert max(worst.values()) <= TOL, worst


# ------------------------------------------------------------------ naive string
def test_naive_string_matches_reference():
    s = ska.random_sequences(2, 40, 77)
    strs = ["", "A", "AC", s[0], s[1], "ACGUNRYACGU-ACGU"]
    o, r = [], []
    for a in strs:
        for b in strs:
            for g in (0.8, 0.55):
                o.append(po.naive_string(a, b, g))
                r.append(po.ref_naive_string(a, b, g))
    w = refdp.worst_rel(o, r)
    print("naive string worst rel:", w)
    assert w <= TOL


# ------------------------------------------------------------------ 4-D and PairHMM
_CFG4D = {
    "full_dp": {},
    "full_dp bp_bound params": dict(bp_bound=0.05, gap=0.6, stack=1.2, subst=0.4),
    "full_dp NormalBasePair": dict(model=1, bp_bound=0.5),
    "full_dp WobbleBasePair": dict(model=2, bp_bound=0.5, loop=4),
    "partial_dp band 2": dict(band=2),
    "partial_dp band 5": dict(band=5),
    "partial_dp band 3 WobbleBasePair": dict(model=2, bp_bound=0.5, band=3),
    "partial_dp ali_bound": dict(ali_bound=0.3),
    "partial_dp ali_bound band 2": dict(ali_bound=0.5, band=2),
}


@pytest.mark.parametrize("cfg", list(_CFG4D))
def test_stem4d_matches_reference(cfg):
    """full_dp, and partial_dp under -b bands and under the -a constraints as
    the reference computes them when built today (LogValue's zerop is never
    true with a C++11 <cmath>: the oracle's zerop_fixed = 0)."""
    kw = _CFG4D[cfg]
    seqs = [s.lower() for s in refdp.stem4d_seqs()]
    if "band" not in kw and "ali_bound" not in kw:
        seqs.append("")  # partial_dp reads c_high[j-1] of an empty constraint vector
    bps = [ska.fold(s) if s else np.zeros(0) for s in seqs]
    o, r = [], []
    for i, x in enumerate(seqs):
        for j, y in enumerate(seqs):
            o.append(po.stem4d(x, bps[i], y, bps[j], zerop_fixed=0, **kw))
            r.append(po.ref_stem4d(x, bps[i], y, bps[j], **kw))
    w = refdp.worst_rel(o, r)
    print(cfg, "worst rel:", w, "largest K:", max(r))
    if kw.get("model", 0) == 0:
        assert max(r) > 1.0  # stacking terms reach the value
    assert w <= TOL


def test_phmm_posteriors_and_constraints_match_reference():
    """PairHMM forward-backward posteriors, and the constraint vectors of
    alignment_constraints (MAP path, anchors, band).  As built with a C++11
    <cmath> the reference's posteriors are NaN and anchor nothing: the oracle
    reproduces exactly that with zerop_fixed = 0, which is what is pinned
    here; the intended semantics (zerop_fixed = 1) has no reference build to
    compare with."""
    seqs = [s.lower() for s in refdp.stem4d_seqs()]
    for x in seqs:
        for y in seqs:
            fo, fr = po.phmm_posterior(x, y, 0), po.ref_phmm_posterior(x, y)
            assert np.array_equal(fo, fr, equal_nan=True), (x, y)
            for ab, band in ((0.3, 0), (0.5, 2), (0.9, 5), (0.0, 2), (0.0, 5)):
                lo, hi = po.alignment_constraints(x, y, ab, band, 0)
                rlo, rhi = po.ref_alignment_constraints(x, y, ab, band)
                assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi), (x, y, ab, band)


# ------------------------------------------------------------------ BPLA
def _bpla_examples(use_bp):
    om, rb = [], []
    for rows in refdp.bpla_alignments():
        bpps = refdp.fold_rows(rows) if use_bp else None
        om.append(po.OMData(rows, bpps, 0.01, use_bp))
        rb.append(po.RBData(rows, bpps, use_bp))
    return om, rb


def test_bpla_weights_match_reference():
    """fill_weight of bpla_kernel/data.cpp, run by the reference's own Data
    constructor on the injected table."""
    om, rb = _bpla_examples(True)
    for o, r in zip(om, rb):
        for a, b in zip(po.bpla_weights(o), r.weights()):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("sw", [False, True])
@pytest.mark.parametrize("no_bp", [False, True])
def test_bpla_values_match_reference(no_bp, sw):
    om, rb = _bpla_examples(not no_bp)
    p = ska.BPLAKernel(noBP=no_bp, SW=sw, alpha=2.0, beta=0.2, gap=-6.0, ext=-0.5).params
    t = list(p.score_table)
    n = len(om)
    o = [[po.bpla(om[i], om[j], no_bp, sw, p.gap, p.ext, p.alpha, p.beta, t) for j in range(n)]
         for i in range(n)]
    r = [[po.ref_bpla(rb[i], rb[j], no_bp, sw, p.gap, p.ext, p.alpha, p.beta, t) for j in range(n)]
         for i in range(n)]
    w = refdp.worst_rel(o, r)
    print(f"BPLA no_bp={no_bp} sw={sw} worst rel:", w)
    assert w <= TOL


def test_bpla_gradients_match_reference():
    """compute_gradients: the value and d/d(alpha, beta, gap, ext)."""
    om, rb = _bpla_examples(True)
    p = ska.BPLAKernel(alpha=2.0, beta=0.2).params
    t = np.array(list(p.score_table))
    n = len(om)
    o, r = [], []
    for i in range(n):
        for j in range(n):
            v, d, _ = po.bpla_gradients(om[i], om[j], p.alpha, p.beta, p.gap, p.ext, t)
            rv, rd = po.ref_bpla_gradients(rb[i], rb[j], p.alpha, p.beta, p.gap, p.ext, t)
            o.append([v, *d])
            r.append([rv, *rd])
    o, r = np.array(o), np.array(r)
    worst = [refdp.worst_rel(o[:, k], r[:, k]) for k in range(5)]
    print("BPLA worst rel (value, d_alpha, d_beta, d_gap, d_ext):", worst)
    assert np.any(r[:, 3] != 0.0) and np.any(r[:, 4] != 0.0)
    assert max(worst) <= TOL
