"""Gradients of the DAG stem kernels, host side.  The long-double restatement
with tangents (tests/stem_grad_ref.py) against the oracle's su_stem_ld /
si_stem_ld (value) and Richardson-extrapolated central differences of them
(derivatives); the host path (sk_stem_gradients_host) against the oracle bit
for bit (value) and against the restatement (derivatives); the composite
kinds, the refusals, the normalised gradient Gram and optimize_stem on a toy
set.  No GPU.

Host derivatives against the restatement, err = |a - b| / (|b| + |K|), the
worst over REF_PAIRS and the eight configurations, measured on this code
(test_host_derivatives prints them):
    loop_gap 2.34e-15   beta 1.46e-15   stack 4.3e-16   covar 1.34e-15
The gate is 16 x the worst of them (rounding differs by pair and parameter),
far inside the 1e-9 it may never exceed."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import stem_grad_ref as R
from tests.helpers import make_examples, mutate_alignment

_I32P = C.POINTER(C.c_int32)
_F64P = C.POINTER(C.c_double)

SEQ_LENS = (24, 27, 30, 33, 36, 40, 45, 50, 55, 60)
ALN_LENS = (30, 36, 42, 48)
EMPTY = 14  # the example with no base pair above th
N_EX = 15
LOOP_GAPS = (0.2, 0.98)
BANDS = (10, 0)
# ordered pairs the long-double restatement is computed for: sequence x
# sequence, alignment x alignment, mixed, a diagonal cell, the empty DAG
REF_PAIRS = ((0, 1), (2, 5), (9, 3), (4, 4), (10, 11), (12, 6), (7, 13), (13, 10), (8, 9), (EMPTY, 2), (3, EMPTY))
MEASURED_WORST = 2.34e-15
HOST_GATE = min(16 * MEASURED_WORST, 1e-9)


def examples():
    seqs = [ska.random_sequences(1, n, 0x57E6 + n)[0] for n in SEQ_LENS]
    alns = [mutate_alignment(ska.random_sequences(1, n, 0xA11 + n)[0], 3, 100 + n, gap=0.08) for n in ALN_LENS]
    return seqs + alns + ["A" * 26]


def kernel(subst, loop_gap, band):
    return ska.SuStemKernel(loop_gap=loop_gap, len_band=band) if subst else \
        ska.SiStemKernel(loop_gap=loop_gap, len_band=band)


def configs():
    return list(itertools.product((True, False), LOOP_GAPS, BANDS))


def ref_pair(ex, subst, p, i, j):
    if subst:
        return R.su(ex[i], ex[j], p.loop_gap, p.beta, p.len_band)
    return R.si(ex[i], ex[j], p.loop_gap, p.stack, p.covar, p.len_band)


def oracle_ld(om, subst, i, j, loop_gap, a, b, band):
    if subst:
        return po.su_stem_ld(om[i], om[j], loop_gap, a, band)
    return po.si_stem_ld(om[i], om[j], loop_gap, a, b, band)


@pytest.fixture(scope="module")
def data():
    ex = examples()
    assert any("-" in r for a in ex[10:14] for r in a), "the alignments need gap columns"
    ds, om = make_examples(ex)
    assert len(om) == N_EX
    return ds, om, [R.Ex(o) for o in om]


@pytest.fixture(scope="module")
def ref(data):
    """The restatement's [K, tangents] of REF_PAIRS for every configuration,
    computed once."""
    _, _, ex = data
    out = {}
    for subst, g, band in configs():
        p = kernel(subst, g, band).params
        for i, j in REF_PAIRS:
            out[subst, g, band, i, j] = ref_pair(ex, subst, p, i, j)
    return out


def all_pairs(n):
    x, y = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return x.ravel().astype(np.int32), y.ravel().astype(np.int32)


def test_fixture_shapes(data):
    _, om, ex = data
    assert ex[EMPTY].n == 0
    assert all(e.n > 0 for e in ex[:EMPTY])


def test_restatement_value_is_the_oracles(data, ref):
    _, om, _ = data
    worst = 0.0
    for (subst, g, band, i, j), r in ref.items():
        p = kernel(subst, g, band).params
        o = oracle_ld(om, subst, i, j, g, p.beta if subst else p.stack, p.covar, band)
        u = R.ulp_diff(np.float64(r[0]), o)
        worst = max(worst, u)
        assert u <= 2, (subst, g, band, i, j, float(r[0]), o)
    print("restatement value against the oracle's long double: worst", worst, "ulp")


def test_restatement_derivatives_are_central_differences(data, ref):
    """(4 D(h/2) - D(h)) / 3 of the oracle's long-double value, h = 1e-4,
    within 1e-8 (|d| + |K|)."""
    _, om, _ = data
    h = 1e-4
    worst = 0.0
    for (subst, g, band, i, j), r in ref.items():
        p = kernel(subst, g, band).params
        base = [g, p.beta] if subst else [g, p.stack, p.covar]

        def f(k, dv):
            q = list(base)
            q[k] += dv
            return oracle_ld(om, subst, i, j, q[0], q[1], q[2] if len(q) > 2 else 0.0, band)

        for k in range(len(base)):
            d1 = (f(k, h) - f(k, -h)) / (2 * h)
            d2 = (f(k, h / 2) - f(k, -h / 2)) / h
            rich = (4 * d2 - d1) / 3
            d = float(r[1 + k])
            tol = 1e-8 * (abs(rich) + abs(float(r[0])))
            if tol > 0:
                worst = max(worst, abs(d - rich) / (abs(rich) + abs(float(r[0]))))
            assert abs(d - rich) <= tol, (subst, g, band, i, j, k, d, rich)
    print("restatement derivatives against Richardson differences: worst", worst)


def test_host_value_is_the_oracles_bit_for_bit(data):
    ds, om, _ = data
    x, y = all_pairs(N_EX)
    for subst, g, band in configs():
        kern = kernel(subst, g, band)
        p = kern.params
        val, grad = ska.stem_gradients(ds, kern, x, y, n_threads=4)
        for k in range(x.size):
            o = po.su_stem(om[x[k]], om[y[k]], g, p.beta, band) if subst else \
                po.si_stem(om[x[k]], om[y[k]], g, p.stack, p.covar, band)
            assert val[k] == o, (subst, g, band, x[k], y[k], val[k], o)
        dead = grad[:, 2:4] if subst else grad[:, 1:2]
        assert not dead.any() and not np.signbit(dead).any()
        e = (x == EMPTY) | (y == EMPTY)
        assert not val[e].any() and not grad[e].any() and not np.signbit(grad[e]).any()
        assert np.signbit(val[e]).sum() == 0
        # one thread and many give the same bits
        v1, g1 = ska.stem_gradients(ds, kern, x[:40], y[:40], n_threads=1)
        assert np.array_equal(v1, val[:40]) and np.array_equal(g1, grad[:40])


def test_host_derivatives(data, ref):
    ds, _, _ = data
    names = ("loop_gap", "beta", "stack", "covar")
    worst = dict.fromkeys(names, 0.0)
    px = np.array([i for i, _ in REF_PAIRS], np.int32)
    py = np.array([j for _, j in REF_PAIRS], np.int32)
    bad = []
    for subst, g, band in configs():
        val, grad = ska.stem_gradients(ds, kernel(subst, g, band), px, py)
        for k, (i, j) in enumerate(REF_PAIRS):
            r = ref[subst, g, band, i, j]
            want = R.row4(subst, r)
            for s in range(4):
                den = abs(float(want[s])) + abs(float(r[0]))
                err = abs(grad[k, s] - float(want[s])) / den if den else abs(grad[k, s])
                worst[names[s]] = max(worst[names[s]], err)
                if not err <= HOST_GATE:
                    bad.append((subst, g, band, i, j, names[s], err))
    print("host derivatives against the restatement, worst err per parameter:", worst, "gate", HOST_GATE)
    assert not bad, bad


def test_composite_kinds(data):
    ds, om, _ = data
    x = np.array([0, 5, 11, 9, EMPTY, 3], np.int32)
    y = np.array([1, 5, 12, 2, 4, EMPTY], np.int32)
    su, si = ska.SuStemKernel(), ska.SiStemKernel()
    v0, g0 = ska.stem_gradients(ds, su, x, y)
    v1, g1 = ska.stem_gradients(ds, si, x, y)
    # + string: the stem part's gradient bit for bit, the value with the string term
    v4, g4 = ska.stem_gradients(ds, ska.SuStemStrKernel(), x, y)
    v5, g5 = ska.stem_gradients(ds, ska.SiStemStrKernel(), x, y)
    assert np.array_equal(g4, g0) and np.array_equal(g5, g1)
    for k in range(x.size):
        for v, kern in ((v4, ska.SuStemStrKernel()), (v5, ska.SiStemStrKernel())):
            o = po.kernel_value(kern.params.kind, om[x[k]], om[y[k]], kern.params)
            assert v[k] == o, (k, v[k], o)
    # log kinds: V = beta log Ks, d/dloop_gap = beta Ks'/Ks, d/dbeta = log Ks + beta dKs/Ks
    beta = su.params.beta
    ok = v0 > 0
    assert ok.sum() == 4
    v6, g6 = ska.stem_gradients(ds, ska.LSuStemKernel(), x, y)
    v7, g7 = ska.stem_gradients(ds, ska.LSuStemStrKernel(), x, y)
    for k in np.flatnonzero(ok):
        lk = math.log(v0[k])
        assert v6[k] == pytest.approx(beta * lk, rel=4e-16)
        assert g6[k, 0] == beta * g0[k, 0] / v0[k]
        assert g6[k, 1] == pytest.approx(lk + beta * g0[k, 1] / v0[k], rel=4e-16)
        assert g6[k, 2] == 0.0 and g6[k, 3] == 0.0
        o = po.kernel_value(7, om[x[k]], om[y[k]], ska.LSuStemStrKernel().params)
        assert v7[k] == pytest.approx(o, rel=1e-14)
    assert np.array_equal(g7, g6, equal_nan=True)
    # Ks = 0: the value sk_pairs returns and no derivative
    for k in np.flatnonzero(~ok):
        assert v6[k] == -np.inf and v7[k] == -np.inf
        assert np.isnan(g6[k, 0]) and np.isnan(g6[k, 1]) and g6[k, 2] == 0.0 and g6[k, 3] == 0.0
    with pytest.raises(ValueError):
        ska.stem_gradient_gram(ds, ska.LSuStemKernel())


def _host_call(xs, ys, kern, x, y):
    x = np.ascontiguousarray(x, np.int32)
    y = np.ascontiguousarray(y, np.int32)
    val = np.zeros(max(x.size, 1))
    grad = np.zeros(4 * max(x.size, 1))
    return ska.lib().sk_stem_gradients_host(xs.handle, ys.handle, C.byref(kern.params), x.ctypes.data_as(_I32P),
                                            y.ctypes.data_as(_I32P), x.size, 1, val.ctypes.data_as(_F64P),
                                            grad.ctypes.data_as(_F64P))


def test_refusals():
    ds, _ = make_examples(ska.random_sequences(3, 24, 5))
    nobp, _ = make_examples(ska.random_sequences(2, 24, 6), use_bp=False)
    su = ska.SuStemKernel()
    assert _host_call(ds, ds, su, [0], [2]) == 0
    # any other kind
    for kern in (ska.StringKernel(), ska.StringKernel(match=1.0, mismatch=0.8), ska.NaiveStringKernel(),
                 ska.BPLAKernel(), ska.StemKernel4D(), ska.LAKernel(), ska.SimpalKernel()):
        assert _host_call(ds, ds, kern, [0], [1]) == -1, type(kern).__name__
    # a dataset built with use_bp = 0, on either side
    assert _host_call(nobp, nobp, su, [0], [1]) == -1
    assert _host_call(ds, nobp, su, [0], [1]) == -1
    assert _host_call(nobp, ds, su, [0], [1]) == -1
    # an index outside its dataset
    for x, y in (([3], [0]), ([0], [3]), ([-1], [0]), ([0, 1], [1, -1])):
        assert _host_call(ds, ds, su, x, y) == -5
    assert _host_call(ds, nobp, su, [0], [5]) == -1  # (the dataset is refused first)
    with pytest.raises(ska.StemKernelError) as e:
        ska.stem_gradients(ds, su, [0], [7])
    assert e.value.code == -5
    # refused in Python before any call
    for call in (lambda k: ska.stem_gradients(ds, k, [0], [1]), lambda k: ska.stem_gradient_gram(ds, k),
                 lambda k: ska.stem_auc_objective(ds, k, [1, -1, 1], 2, 1.0),
                 lambda k: ska.optimize_stem(ds, [1, -1, 1], k)):
        with pytest.raises(ValueError):
            call(ska.StringKernel())
    for name in ("stem_gradients", "stem_gradient_gram", "stem_auc_objective"):
        assert hasattr(ska.Context, name)


def test_normalised_gradient_gram(data):
    from stem_kernel_amd.shard import assemble_gradients
    ds, _, _ = data
    sub = ska.Dataset()
    for k, ex in enumerate(examples()[:6]):
        rows = [ex] if isinstance(ex, str) else list(ex)
        sub.add("+1", rows)
    kern = ska.SiStemKernel(loop_gap=0.4)
    n = len(sub)
    iu, ju = np.triu_indices(n)
    val, grad = ska.stem_gradients(sub, kern, iu, ju)
    for normalize in (False, True):
        K, G = ska.stem_gradient_gram(sub, kern, normalize=normalize)
        Kw, Gw = assemble_gradients(iu, ju, val, grad, n, normalize)
        assert np.array_equal(K, Kw) and np.array_equal(G, Gw)
        assert G.shape == (4, n, n) and not G[1].any()
    # the normalised derivative by hand for one cell
    K, G = ska.stem_gradient_gram(sub, kern, normalize=True)
    Ku, Gu = ska.stem_gradient_gram(sub, kern, normalize=False)
    i, j, s = 1, 4, 0
    want = Gu[s, i, j] / math.sqrt(Ku[i, i] * Ku[j, j]) - 0.5 * Ku[i, j] / math.sqrt(Ku[i, i] * Ku[j, j]) * (
        Gu[s, i, i] / Ku[i, i] + Gu[s, j, j] / Ku[j, j])
    assert G[s, i, j] == pytest.approx(want, rel=1e-12)
    assert np.all(np.diag(K) == 1.0) and not np.diagonal(G, axis1=1, axis2=2).any()


def _toy_set():
    """Sixteen labelled examples: two families of mutated hairpin sequences."""
    a = "GGGGCAUCUUCGGAUGCCCCAAGGCCUUAAGGCC"
    b = "AUAUACGCGAAAGCGCGUAUAUUUGCAUGAAAUGCAA"
    seqs, labels = [], []
    for k in range(8):
        seqs.append(mutate_alignment(a, 1, 300 + k, sub=0.08, gap=0.0)[0])
        labels.append(1)
        seqs.append(mutate_alignment(b, 1, 400 + k, sub=0.08, gap=0.0)[0])
        labels.append(-1)
    ds, _ = make_examples(seqs)
    return ds, labels


@pytest.mark.parametrize("subst", [True, False])
def test_optimize_stem_on_a_toy_set(subst):
    pytest.importorskip("scipy")
    ds, labels = _toy_set()
    start = ska.SuStemKernel() if subst else ska.SiStemKernel()
    seen = []
    res, best = ska.optimize_stem(ds, labels, start, C=1.0, n_folds=4, normalize=True, maxiter=3,
                                  callback=lambda step, x, f, g: seen.append((x.copy(), f, g.copy())))
    live = ("loop_gap", "beta") if subst else ("loop_gap", "stack", "covar")
    assert len(seen) >= 1 and all(g.size == 1 + len(live) for _, _, g in seen)
    assert np.array_equal(seen[0][0], [1.0] + [getattr(start.params, s) for s in live])
    assert res.fun <= seen[0][1]
    assert res.x[0] >= 1e-5 and 1e-3 <= res.x[1] <= 1.0 and all(v >= 1e-3 for v in res.x[2:])
    p = best.params
    assert p.kind == start.params.kind and p.len_band == start.params.len_band
    assert tuple(getattr(p, s) for s in live) == tuple(res.x[1:])
