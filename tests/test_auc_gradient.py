"""The optimizer's cross-validated AUC gradient on the GPU
(sk_auc_gradient_batch, csrc/kernels/auc_grad.hip) against the host path
(csrc/host/auc_gradient.cpp) and the reference's own values
(tests/golden/auc_gradient.json), bit for bit: the conjugate gradient on the
indefinite KKT system amplifies rounding, so no tolerance applies -- both
paths keep the reference's order in every sum."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from tests import auc_ref, svm_ref
from tests.auc_ref import as_problem, bits, hexes

pytestmark = pytest.mark.gpu
SHAPE = ska.auc_gradient_shape()
PROBLEMS, MATS = auc_ref.fixture()
N = 400


def assert_same(g, h, what, finite=True):
    """Every output and info field of the GPU result g is the host result h's:
    equal bits where h is a number, a NaN where h has one (a NaN's sign and
    payload are the processor's, not the computation's)."""
    assert (g.n_free, g.n_bound, g.cg_iterations, g.finite) == (h.n_free, h.n_bound, h.cg_iterations, h.finite), \
        (what, g, h)
    assert h.finite == finite, (what, h)
    for name, a, b in (("cg", [g.cg], [h.cg]), ("fg", g.fg, h.fg), ("d_u", g.d_u, h.d_u)):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        assert a.shape == b.shape, (what, name)
        nan = np.isnan(b)
        assert np.array_equal(np.isnan(a), nan), (what, name)
        assert np.array_equal(bits(a)[~nan], bits(b)[~nan]), (what, name, a, b)


@pytest.fixture(scope="module")
def crafted():
    """A 400-example integer Gram with a ridge (so that the free block is
    definite and the system regular), three gradient matrices from other
    seeds, and one crafted problem per free count: the edges of a wave, of the
    LDS / scratch cutoff, and 300 (several rows per thread in the LDS class's
    neighbour).  Host results computed once."""
    K, y = svm_ref.int_gram(0x5A17D001, N, 24, 4)
    K = K + 2.0 * np.eye(N)
    G = np.stack([svm_ref.int_gram(0x5A17D010 + k, N, 24, 4)[0] for k in range(3)])
    tr, ts = svm_ref.split(N, 5, 0)
    cut = SHAPE["lds_free"]
    frees = [0, 1, 2, 63, 64, 65, cut, cut + 1, 300]
    ps = []
    for nf in frees:
        alpha, rho, dec = auc_ref.crafted(0xB000 + nf, tr, ts, 1.5, nf, 10)
        _, delta = ska.auc_delta(dec, y[ts])
        ps.append(dict(train=tr, test=ts, C=1.5, alpha=alpha, rho=rho, delta=delta))
    host = ska.auc_gradient_batch(K, G, y, ps)
    assert [h.n_free for h in host] == frees and all(h.n_bound == 10 for h in host)
    return K, G, y, frees, ps, host


def test_shape():
    assert 100 <= SHAPE["lds_free"] < SHAPE["max_free"] and SHAPE["max_free"] >= 1024
    assert 8 * (SHAPE["max_free"] + 1) ** 2 <= SHAPE["scratch_budget"]


def test_free_counts_one_problem_per_call(gpu_ctx, crafted):
    K, G, y, frees, ps, host = crafted
    for nf, p, h in zip(frees, ps, host):
        g = ska.auc_gradient_batch(K, G, y, [p], ctx=gpu_ctx)[0]
        assert gpu_ctx.last_launch_ms()["launches"] == 1
        assert_same(g, h, f"n_free = {nf}")
        assert h.cg_iterations >= min(nf, 2), (nf, h)  # the conjugate gradient ran


def test_mixed_batch_and_its_reverse(gpu_ctx, crafted):
    """All sizes in one call (both classes: two launches), and the same
    batch reversed: the problems share no state."""
    K, G, y, frees, ps, host = crafted
    gpu = ska.auc_gradient_batch(K, G, y, ps, ctx=gpu_ctx)
    assert gpu_ctx.last_launch_ms()["launches"] == 2
    rev = ska.auc_gradient_batch(K, G, y, ps[::-1], ctx=gpu_ctx)[::-1]
    for nf, g, r, h in zip(frees, gpu, rev, host):
        assert_same(g, h, f"mixed, n_free = {nf}")
        assert_same(r, h, f"reversed, n_free = {nf}")


def test_no_gradient_matrices(gpu_ctx, crafted):
    K, _, y, frees, ps, host = crafted
    sel = [1, 5, 8]
    gpu = ska.auc_gradient_batch(K, None, y, [ps[k] for k in sel], ctx=gpu_ctx)
    for k, g in zip(sel, gpu):
        assert len(g.fg) == 0 and bits([g.cg])[0] == bits([host[k].cg])[0]
        assert np.array_equal(bits(g.d_u), bits(host[k].d_u))


def test_fixture_problems(gpu_ctx):
    """The reference's own d_u, cg and fg, bit for bit, from the fixture's
    alpha, rho and delta; one call per (Gram, gradient matrices)."""
    groups = {}
    for p in PROBLEMS:
        groups.setdefault((p["k"], tuple(p["g"])), []).append(p)
    for ps in groups.values():
        K, G, y = auc_ref.inputs(ps[0], MATS)
        gpu = ska.auc_gradient_batch(K, G, y, [as_problem(p) for p in ps], ctx=gpu_ctx)
        for p, g in zip(ps, gpu):
            assert (g.n_free, g.n_bound, g.cg_iterations) == (p["n_free"], p["n_bound"], p["cg_iterations"]), p["name"]
            assert g.finite, p["name"]
            assert np.array_equal(bits(g.d_u), bits(hexes(p["d_u"]))), p["name"]
            assert bits([g.cg])[0] == bits([float.fromhex(p["cg"])])[0], p["name"]
            assert np.array_equal(bits(g.fg), bits(hexes(p["fg"]))), p["name"]


def zero_division_case():
    """A conjugate gradient that divides by zero: one free example u whose
    diagonal entry is 0 in an indefinite integer Gram, and weights delta
    that sum to exactly 0, so w.z = K_uu w_0^2 - 2 y w_0 w_1 = 0 while r.r is
    far above the tolerance."""
    K, y = svm_ref.int_gram(0x5A17A102, 60, 4, 0, 1, 0)
    u = next(k for k in range(60) if K[k, k] == 0 and np.any(K[k] != 0))
    tr = np.array([t for t in range(60) if t % 5 != 4 or t == u][:48])
    ts = np.array([t for t in range(60) if t not in set(tr.tolist())])
    delta = np.zeros(len(ts))
    other = next(j for j in range(len(ts)) if K[u][ts[j]] != K[u][ts[0]])
    delta[0], delta[other] = 0.5, -0.5
    alpha = np.zeros(len(tr))
    alpha[:3] = 1.0
    alpha[tr.tolist().index(u)] = 0.5
    G = np.stack([K.T * 0.5, K + 1.0])
    return K, G, y, dict(train=tr, test=ts, C=1.0, alpha=alpha, rho=0.25, delta=delta)


def test_division_by_zero_propagates_and_ends(gpu_ctx):
    K, G, y, p = zero_division_case()
    h = ska.auc_gradient_batch(K, G, y, [p])[0]
    assert h.n_free == 1 and not h.finite and np.isnan(h.cg) and np.all(np.isnan(h.d_u))
    assert h.cg_iterations == h.n_free + 2  # no stopping test passes on a NaN: every pass runs
    g = ska.auc_gradient_batch(K, G, y, [p], ctx=gpu_ctx)[0]
    assert_same(g, h, "division by zero", finite=False)


def test_over_the_scratch_budget_is_unsupported_before_any_launch(gpu_ctx, crafted):
    K, G, y, _, ps, _ = crafted
    ska.auc_gradient_batch(K, G, y, ps[:1], ctx=gpu_ctx)
    assert gpu_ctx.last_launch_ms()["launches"] == 1
    n = SHAPE["max_free"] + 8
    big_y = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    tr = np.arange(SHAPE["max_free"] + 1, dtype=np.int32)
    too_big = dict(train=tr, test=[n - 2, n - 1], C=1.0, alpha=np.full(len(tr), 0.5), rho=0.0, delta=[0.5, -0.5])
    with pytest.raises(ska.StemKernelError) as e:
        ska.auc_gradient_batch(np.zeros((n, n)), None, big_y, [too_big], ctx=gpu_ctx)
    assert e.value.code == -6 and gpu_ctx.last_launch_ms()["launches"] == 0


def test_errors_return_before_any_launch(gpu_ctx, crafted):
    K, G, y, _, ps, _ = crafted
    bad = dict(ps[1], C=0.0)
    ska.auc_gradient_batch(K, G, y, ps[:1], ctx=gpu_ctx)
    assert gpu_ctx.last_launch_ms()["launches"] == 1
    with pytest.raises(ska.StemKernelError) as e:
        ska.auc_gradient_batch(K, G, y, [ps[0], bad], ctx=gpu_ctx)
    assert e.value.code == -1 and gpu_ctx.last_launch_ms()["launches"] == 0


def test_objective_end_to_end(gpu_ctx):
    """auc_objective on the GPU over the RBF Gram (gamma the one parameter).
    Training gives the host path's alpha and rho bit for bit, but the GPU's
    decision values are summed in another order than the host's, so delta --
    and with it g -- need not be the host path's bits.  What is asserted:
    (1) fed the same delta (the host's), the GPU gradient is the host's bit
    for bit in every fold; (2) the GPU objective's g is, bit for bit, the
    host path's gradient of the GPU's own delta summed in fold order; (3)
    where every fold's GPU decision values are the host's bits, f and g are
    the host objective's bits."""
    K, y = MATS[4]
    G = np.stack([MATS[5][0]])
    for C in (1.0, 64.0):
        fh, gh, rh = ska.auc_objective(K, G, y, 5, C)
        fg_, gg, rg = ska.auc_objective(K, G, y, 5, C, ctx=gpu_ctx)
        assert np.isfinite(fg_) and np.all(np.isfinite(gg))
        folds = [ska.cv_split(40, 5, f) for f in range(5)]
        for a, b in zip(rh, rg):
            assert np.array_equal(bits(a["solution"].alpha), bits(b["solution"].alpha))
            assert bits([a["solution"].rho])[0] == bits([b["solution"].rho])[0]
        same_delta = [dict(train=tr, test=ts, C=C, alpha=a["solution"].alpha, rho=a["solution"].rho, delta=a["delta"])
                      for (tr, ts), a in zip(folds, rh)]
        for a, g in zip(rh, ska.auc_gradient_batch(K, G, y, same_delta, ctx=gpu_ctx)):
            assert_same(g, a["gradient"], f"C = {C}, host delta")
        own = [dict(train=tr, test=ts, C=C, alpha=b["solution"].alpha, rho=b["solution"].rho, delta=b["delta"])
               for (tr, ts), b in zip(folds, rg)]
        want = np.zeros(2)
        for h in ska.auc_gradient_batch(K, G, y, own):
            want[0] -= h.cg
            want[1] -= h.fg[0]
        assert np.array_equal(bits(gg), bits(want)), (C, gg, want)
        if all(np.array_equal(bits(a["solution"].decision), bits(b["solution"].decision)) for a, b in zip(rh, rg)):
            assert bits([fg_])[0] == bits([fh])[0] and np.array_equal(bits(gg), bits(gh))


def test_bpla_auc_objective(gpu_ctx):
    """One step of the bpla_optimizer on the GPU: the Gram and its four
    gradient matrices, the folds' training and the AUC gradient.  The
    composition is auc_objective over bpla_gradient_gram, bit for bit."""
    from tests.helpers import make_examples, mutate_alignment
    alns = [mutate_alignment(s, 2, 71 + k) for k, s in enumerate(ska.random_sequences(12, 30, 71))]
    ds, _ = make_examples(alns)
    kern = ska.BPLAKernel()
    labels = np.where(np.arange(12) % 4 < 2, 1.0, -1.0)  # both classes in every fold's two lists
    f, g, rec = gpu_ctx.bpla_auc_objective(ds, kern, labels, 3, 2.0, normalize=True)
    assert np.isfinite(f) and g.shape == (5,) and len(rec) == 3
    K, G = gpu_ctx.bpla_gradient_gram(ds, kern, normalize=True)
    f2, g2, _ = ska.auc_objective(K, G, labels, 3, 2.0, ctx=gpu_ctx)
    assert bits([f])[0] == bits([f2])[0]
    nan = np.isnan(g2)
    assert np.array_equal(np.isnan(g), nan) and np.array_equal(bits(g)[~nan], bits(g2)[~nan])
    assert -3.0 <= f <= 0.0  # minus the sum of three smoothed AUCs
