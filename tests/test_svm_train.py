"""C-SVC training on the GPU (csrc/kernels/svm_smo.hip, sk_svm_train_batch)
against the fixture tests/golden/svm_train.json (the reference's own solver)
and against the host path (csrc/host/svm_train.cpp), which
tests/test_svm_train_cpu.py pins to that fixture.  Alphas are compared bit for
bit.  Every problem carries max_iter <= 200,000; the host path needs at most
some 37,000 iterations on any of them."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from tests import svm_ref
from tests.svm_ref import BAD, as_problem, bits, hexes, one_class_lists

pytestmark = pytest.mark.gpu
CAP = 200_000
SHAPE = ska.svm_train_shape()
PROBLEMS, GRAMS = svm_ref.fixture()


def capped(p):
    q = dict(p)
    q["max_iter"] = min(q.get("max_iter", CAP), CAP)
    return q


def assert_same_solution(g, h, what):
    """GPU solution g against host solution h: everything the solve determines."""
    assert np.array_equal(bits(g.alpha), bits(h.alpha)), (what, np.flatnonzero(bits(g.alpha) != bits(h.alpha))[:8])
    assert (g.iterations, g.status, g.n_free, g.n_bound) == (h.iterations, h.status, h.n_free, h.n_bound), what


def assert_sums_close(K, y, g, h, what):
    """rho and obj: one thread adds their terms in index order, so they are
    the host path's bits (and with that inside 2 l 2^-53 sum |term|, asserted
    too).  Decision values: within 2 l 2^-53 sum |term| of the sequential sum
    (the host path's), plus the two paths' roundings of the final `- rho`."""
    t, l = h.train, len(h.train)
    rho_b, obj_b = svm_ref.sum_bounds(K, y, t, h.Cp, h.Cn, h.alpha, 2 * l * 2.0 ** -53)
    print(f"{what}: |rho - host| {abs(g.rho - h.rho):.3g} (bound {rho_b:.3g}), |obj - host| "
          f"{abs(g.obj - h.obj):.3g} (bound {obj_b:.3g})", end="")
    assert abs(g.rho - h.rho) <= rho_b and abs(g.obj - h.obj) <= obj_b, what
    assert g.rho == h.rho and g.obj == h.obj, what
    if len(h.test):
        terms = np.abs(K[np.ix_(h.test, t)]) @ h.alpha  # sum_a |alpha_a y_a K[s][t_a]|
        dec_b = 2 * l * 2.0 ** -53 * terms + 2.0 ** -53 * (np.abs(g.decision) + np.abs(h.decision))
        err = np.abs(g.decision - h.decision)
        print(f", decision values worst {err.max():.3g} of bound {dec_b[err.argmax()]:.3g}", end="")
        assert np.all(np.isfinite(g.decision)) and np.all(err <= dec_b), what
    print()


def test_fixture_problems(gpu_ctx):
    """The reference solver's alphas, bit for bit; iterations and status as the host path."""
    for gi, (K, y) in enumerate(GRAMS):
        ps = [p for p in PROBLEMS if p["gram"] == gi]
        batch = [capped(dict(as_problem(p), test=list(range(len(y))))) for p in ps]
        gpu = ska.svm_train_batch(K, y, batch, ctx=gpu_ctx)
        host = ska.svm_train_batch(K, y, batch)
        for p, g, h in zip(ps, gpu, host):
            assert np.array_equal(bits(g.alpha), bits(hexes(p["alpha"]))), p["name"]
            assert g.iterations == h.iterations == p["iterations"] and g.status == h.status, p["name"]
            assert_same_solution(g, h, p["name"])
            assert_sums_close(K, y, g, h, p["name"])


@pytest.fixture(scope="module")
def big():
    """An integer Gram as large as the GPU solver's longest training list."""
    return svm_ref.int_gram(0x5A17C001, SHAPE["max_train"], 8, 2)


def test_edges_of_the_size_classes(gpu_ctx, big):
    K, y = big
    b = SHAPE["bounds"]
    assert b[-1] == SHAPE["max_train"] >= 4096
    ls = [2, 3, 63, 64, 65] + [v for e in b[:-1] for v in (e - 1, e, e + 1)] + [b[-1] - 1, b[-1]]
    batch = [dict(train=np.arange(l), test=[0, 1, l // 2], C=0.25, eps=1e-3, max_iter=CAP) for l in ls]
    gpu = ska.svm_train_batch(K, y, batch, ctx=gpu_ctx)
    assert gpu_ctx.last_launch_ms()["launches"] == len(b)  # one launch per class in use
    host = ska.svm_train_batch(K, y, batch)
    for l, g, h in zip(ls, gpu, host):
        assert h.status == "converged" and 1 <= h.iterations < CAP // 5, (l, h)
        assert_same_solution(g, h, f"l = {l}")
        assert_sums_close(K, y, g, h, f"l = {l}")


def test_longer_list_is_unsupported_before_any_launch(gpu_ctx):
    K, y = GRAMS[0]
    ok = dict(train=np.arange(300), C=0.125)
    ska.svm_train_batch(K, y, [ok], ctx=gpu_ctx)
    assert gpu_ctx.last_launch_ms()["launches"] == 1
    too_long = dict(train=np.arange(SHAPE["max_train"] + 1) % 300, C=0.125)
    with pytest.raises(ska.StemKernelError) as e:
        ska.svm_train_batch(K, y, [ok, too_long], ctx=gpu_ctx)
    assert e.value.code == -6 and gpu_ctx.last_launch_ms()["launches"] == 0
    # the longest list itself runs (repeated examples: identical pairs on the TAU path)
    longest = dict(train=np.arange(SHAPE["max_train"]) % 300, C=2.0 ** -6, max_iter=300)
    g = ska.svm_train_batch(K, y, [longest], ctx=gpu_ctx)[0]
    assert_same_solution(g, ska.svm_train_batch(K, y, [longest])[0], "longest list, repeated examples")


def test_iteration_cap(gpu_ctx):
    p = next(p for p in PROBLEMS if p["max_iter"] == 7)
    K, y = GRAMS[p["gram"]]
    for cap in (1, 7, 8):
        q = dict(as_problem(p), max_iter=cap, test=[0, 5])
        g = ska.svm_train_batch(K, y, [q], ctx=gpu_ctx)[0]
        h = ska.svm_train_batch(K, y, [q])[0]
        assert g.status == "not converged" and g.iterations == cap
        assert_same_solution(g, h, f"max_iter {cap}")
        assert_sums_close(K, y, g, h, f"max_iter {cap}")
        if cap == 7:
            assert np.array_equal(bits(g.alpha), bits(hexes(p["alpha"])))


def test_batch_independence(gpu_ctx):
    """40 problems (5 folds x 8 values of C) in one call, one per call, and reversed."""
    K, y = GRAMS[0]
    ps = [dict(train=tr, test=ts, C=2.0 ** e, eps=1e-3, max_iter=CAP)
          for e in range(-4, 4) for tr, ts in (svm_ref.split(len(y), 5, f) for f in range(5))]
    assert len(ps) == 40
    together = ska.svm_train_batch(K, y, ps, ctx=gpu_ctx)
    backwards = ska.svm_train_batch(K, y, ps[::-1], ctx=gpu_ctx)[::-1]
    host = ska.svm_train_batch(K, y, ps)
    for k, p in enumerate(ps):
        alone = ska.svm_train_batch(K, y, [p], ctx=gpu_ctx)[0]
        for other in (together[k], backwards[k]):
            assert_same_solution(other, alone, k)
            assert (other.rho, other.obj) == (alone.rho, alone.obj)
            assert np.array_equal(bits(other.decision), bits(alone.decision))
        assert_same_solution(alone, host[k], k)
    cv = ska.cross_validate(K, y, 5, [2.0 ** e for e in range(-4, 4)], max_iter=CAP, ctx=gpu_ctx)
    for k, s in enumerate(s for row in cv.solutions for s in row):
        assert np.array_equal(bits(s.alpha), bits(together[k].alpha))


DEGENERATE = ["identical pair, l = 2 (TAU)", "identical pair inside", "indefinite C=1", "indefinite C=64",
              "int300 Cp != Cn", "rbf Cp != Cn", "permuted list", "partial list"]


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_inputs(gpu_ctx, name):
    p = next(p for p in PROBLEMS if p["name"] == name)
    K, y = GRAMS[p["gram"]]
    q = capped(dict(as_problem(p), test=list(range(len(y)))))
    g = ska.svm_train_batch(K, y, [q], ctx=gpu_ctx)[0]
    h = ska.svm_train_batch(K, y, [q])[0]
    assert h.status == "converged"
    assert_same_solution(g, h, name)
    assert_sums_close(K, y, g, h, name)


def test_asymmetric_gram_is_read_by_row(gpu_ctx):
    """The DAG kernels are not symmetric before mirroring; Q_i comes from row t_i alone."""
    K, y = GRAMS[0]
    A = K.copy()
    A[np.triu_indices(len(y), 1)] *= 0.5  # exact: entries are multiples of 1/4
    q = dict(train=np.arange(0, 300, 2), test=np.arange(1, 300, 2), C=0.5, max_iter=CAP)
    g = ska.svm_train_batch(A, y, [q], ctx=gpu_ctx)[0]
    h = ska.svm_train_batch(A, y, [q])[0]
    assert_same_solution(g, h, "asymmetric")
    assert_sums_close(A, y, g, h, "asymmetric")


def test_errors_return_before_any_launch(gpu_ctx):
    K, y = GRAMS[0]
    good = dict(train=[0, 1, 2])
    for name, bad in {**BAD, **one_class_lists(y)}.items():
        ska.svm_train_batch(K, y, [good], ctx=gpu_ctx)
        assert gpu_ctx.last_launch_ms()["launches"] == 1
        with pytest.raises(ska.StemKernelError) as e:
            ska.svm_train_batch(K, y, [good, bad], ctx=gpu_ctx)
        assert e.value.code == -1, name
        assert gpu_ctx.last_launch_ms()["launches"] == 0, name
