"""C-SVC training with libsvm's shrinking on the GPU (csrc/kernels/svm_smo.hip,
sk_svm_train_batch_ex) against the fixture tests/golden/svm_train_shrink.json
(the reference's own solver, shrinking = 1) and against the host path
(csrc/host/svm_train.cpp), which tests/test_svm_shrink_cpu.py pins to that
fixture.  Alphas, rho, obj, iterations, status and the counters of
sk_svm_shrink_info are compared bit for bit.  Every problem carries
max_iter <= 200,000; the longest solve here takes some 54,000 iterations."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from tests import svm_ref, svm_shrink_ref
from tests.svm_ref import BAD, as_problem, bits, one_class_lists
from tests.svm_shrink_ref import assert_is_the_record, assert_same

pytestmark = pytest.mark.gpu
CAP = 200_000
SHAPE = ska.svm_train_shape()
PROBLEMS, GRAMS = svm_shrink_ref.fixture()


def capped(p):
    q = dict(p)
    q["max_iter"] = min(q.get("max_iter", CAP), CAP)
    return q


def assert_decision_close(K, g, h, what):
    """Decision values: within 2 l 2^-53 sum |term| of the sequential sum (the
    host path's), plus the two paths' roundings of the final `- rho` -- the
    rule of tests/test_svm_train.py; rho and obj are compared as bits by
    assert_same (one thread adds their terms in position order)."""
    if not len(h.test):
        return
    t, l = h.train, len(h.train)
    terms = np.abs(K[np.ix_(h.test, t)]) @ h.alpha  # sum_a |alpha_a y_a K[s][t_a]|
    dec_b = 2 * l * 2.0 ** -53 * terms + 2.0 ** -53 * (np.abs(g.decision) + np.abs(h.decision))
    err = np.abs(g.decision - h.decision)
    print(f"{what}: decision values worst {err.max():.3g} of bound {dec_b[err.argmax()]:.3g}")
    assert np.all(np.isfinite(g.decision)) and np.all(err <= dec_b), what


@pytest.fixture(scope="module")
def host_fixture():
    """The host path's solutions of the fixture's problems, per Gram, computed once."""
    out = {}
    for gi, (K, y) in enumerate(GRAMS):
        ps = [p for p in PROBLEMS if p["gram"] == gi]
        batch = [capped(dict(as_problem(p), test=list(range(len(y))))) for p in ps]
        out[gi] = (ps, batch, ska.svm_train_batch(K, y, batch, shrinking=True))
    return out


def test_fixture_problems(gpu_ctx, host_fixture):
    """The reference solver's run with shrinking, bit for bit, counters included."""
    for gi, (K, y) in enumerate(GRAMS):
        ps, batch, host = host_fixture[gi]
        gpu = ska.svm_train_batch(K, y, batch, ctx=gpu_ctx, shrinking=True)
        for p, g, h in zip(ps, gpu, host):
            assert_is_the_record(g, p)
            assert_same(g, h, p["name"])
            assert_decision_close(K, g, h, p["name"])


@pytest.fixture(scope="module")
def big():
    """An integer Gram as large as the GPU solver's longest training list."""
    return svm_ref.int_gram(0x5A17C001, SHAPE["max_train"], 8, 2)


def test_edges_of_the_size_classes(gpu_ctx, big):
    K, y = big
    b = SHAPE["bounds"]
    assert b == [256, 1024, 4096] and b[-1] == SHAPE["max_train"]
    cases = [(255, 4.0), (256, 4.0), (257, 4.0), (1023, 4.0), (1024, 4.0), (1025, 4.0), (4096, 1.0)]
    batch = [dict(train=np.arange(l), test=[0, 1, l // 2], C=C, eps=1e-3, max_iter=CAP) for l, C in cases]
    gpu = ska.svm_train_batch(K, y, batch, ctx=gpu_ctx, shrinking=True)
    assert gpu_ctx.last_launch_ms()["launches"] == len(b)  # one launch per class in use
    host = ska.svm_train_batch(K, y, batch, shrinking=True)
    for (l, C), g, h in zip(cases, gpu, host):
        what = f"l = {l}, C = {C:g}"
        # no edge passes without the path: every one of these shrank
        assert h.status == "converged" and h.shrink["shrunk_calls"] >= 1 and h.shrink["min_active"] < l, (what, h.shrink)
        assert_same(g, h, what)
        assert_decision_close(K, g, h, what)
    # the reference's own figures for two of them (its solver, instrumented as the fixture's)
    by = {l: h for (l, _), h in zip(cases, host)}
    assert (by[1025].iterations, by[1025].shrink["shrink_calls"]) == (17845, 17)
    assert by[1025].shrink["unshrunk"] == 1 and by[1025].shrink["regrown"] == 1
    assert (by[4096].iterations, by[4096].shrink["shrink_calls"], by[4096].shrink["resumed"]) == (13591, 14, 1)


def test_iteration_cap(gpu_ctx):
    """Caps that fall while the active set is shrunk, and around them."""
    for name, caps in (("max_iter 250, l = 100", (249, 250, 251)), ("max_iter 700, int300 C=1", (700,)),
                       ("max_iter 7", (1, 7, 8))):
        p = next(p for p in PROBLEMS if p["name"] == name)
        K, y = GRAMS[p["gram"]]
        batch = [dict(as_problem(p), max_iter=cap, test=[0, 5]) for cap in caps]
        gpu = ska.svm_train_batch(K, y, batch, ctx=gpu_ctx, shrinking=True)
        host = ska.svm_train_batch(K, y, batch, shrinking=True)
        for cap, g, h in zip(caps, gpu, host):
            assert g.status == "not converged" and g.iterations == cap
            assert_same(g, h, f"{name}: max_iter {cap}")
            assert_decision_close(K, g, h, f"{name}: max_iter {cap}")
            if cap == p["max_iter"]:
                assert_is_the_record(g, p)


def test_batch_independence(gpu_ctx):
    """40 problems (5 folds x 8 values of C) in one call, one per call, and reversed."""
    K, y = GRAMS[0]
    ps = [dict(train=tr, test=ts, C=2.0 ** e, eps=1e-3, max_iter=CAP)
          for e in range(-4, 4) for tr, ts in (svm_ref.split(len(y), 5, f) for f in range(5))]
    assert len(ps) == 40
    together = ska.svm_train_batch(K, y, ps, ctx=gpu_ctx, shrinking=True)
    backwards = ska.svm_train_batch(K, y, ps[::-1], ctx=gpu_ctx, shrinking=True)[::-1]
    host = ska.svm_train_batch(K, y, ps, shrinking=True)
    assert sum(h.shrink["shrunk_calls"] > 0 for h in host) >= 20
    for k, p in enumerate(ps):
        alone = ska.svm_train_batch(K, y, [p], ctx=gpu_ctx, shrinking=True)[0]
        for other in (together[k], backwards[k]):
            assert_same(other, alone, k)
            assert np.array_equal(bits(other.decision), bits(alone.decision))
        assert_same(alone, host[k], k)
    cv = ska.cross_validate(K, y, 5, [2.0 ** e for e in range(-4, 4)], max_iter=CAP, ctx=gpu_ctx, shrinking=True)
    for k, s in enumerate(s for row in cv.solutions for s in row):
        assert_same(s, together[k], k)


def test_flag_is_per_call(gpu_ctx):
    """The same batch with the flag off is the call without the flag, before
    and after a call with it."""
    K, y = GRAMS[0]
    ps = [capped(dict(as_problem(p), test=[0, 1, 2])) for p in PROBLEMS if p["gram"] == 0 and p["iterations"] < 6000]
    off_before = ska.svm_train_batch(K, y, ps, ctx=gpu_ctx)
    on = ska.svm_train_batch(K, y, ps, ctx=gpu_ctx, shrinking=True)
    off_after = ska.svm_train_batch(K, y, ps, ctx=gpu_ctx, shrinking=False)
    host_off, host_on = ska.svm_train_batch(K, y, ps), ska.svm_train_batch(K, y, ps, shrinking=True)
    differ = 0
    for k, p in enumerate(ps):
        for s in (off_before[k], off_after[k]):
            assert_same(s, host_off[k], k)
            assert s.shrink == dict(shrink_calls=0, shrunk_calls=0, min_active=len(p["train"]), unshrunk=0,
                                    regrown=0, reconstructions=0, resumed=0)
            assert np.array_equal(bits(s.decision), bits(off_before[k].decision))
        assert_same(on[k], host_on[k], k)
        differ += not np.array_equal(bits(on[k].alpha), bits(off_before[k].alpha))
    assert differ >= 5


def test_asymmetric_gram_is_read_by_row(gpu_ctx):
    """Q_i comes from row t_i alone, in the G_bar pass and the reconstruction too."""
    K, y = GRAMS[0]
    A = K.copy()
    A[np.triu_indices(len(y), 1)] *= 0.5  # exact: entries are multiples of 1/4
    # C = 4 does not converge on this matrix (it is no Gram): capped, on a shrunk set
    qs = [dict(train=np.arange(0, 300, 2), test=np.arange(1, 300, 2), C=C, max_iter=cap)
          for C, cap in ((0.25, CAP), (0.5, CAP), (4.0, 5000))]
    gpu = ska.svm_train_batch(A, y, qs, ctx=gpu_ctx, shrinking=True)
    host = ska.svm_train_batch(A, y, qs, shrinking=True)
    assert [h.status for h in host] == ["converged", "converged", "not converged"]
    assert all(h.shrink["reconstructions"] > 0 for h in host[:2]) and all(h.shrink["shrunk_calls"] > 0 for h in host)
    for g, h in zip(gpu, host):
        assert_same(g, h, "asymmetric")
        assert_decision_close(A, g, h, "asymmetric")


def test_errors_return_before_any_launch(gpu_ctx):
    K, y = GRAMS[0]
    good = dict(train=[0, 1, 2])
    for name, bad in {**BAD, **one_class_lists(y)}.items():
        ska.svm_train_batch(K, y, [good], ctx=gpu_ctx, shrinking=True)
        assert gpu_ctx.last_launch_ms()["launches"] == 1
        with pytest.raises(ska.StemKernelError) as e:
            ska.svm_train_batch(K, y, [good, bad], ctx=gpu_ctx, shrinking=True)
        assert e.value.code == -1, name
        assert gpu_ctx.last_launch_ms()["launches"] == 0, name
