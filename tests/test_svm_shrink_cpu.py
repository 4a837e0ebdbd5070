"""C-SVC training with libsvm's shrinking, host path
(sk_svm_train_batch_host_ex): pinned to the reference's own solver run with
shrinking = 1 through tests/golden/svm_train_shrink.json (made by
tools/make_golden_svm_shrink.py from libsvm/solver.cpp compiled in place):
alphas, rho, obj, iterations, status and the seven counters of
sk_svm_shrink_info, bit for bit.  The flag off is the call without it; batch
order; the error codes; cross_validate and auc_objective pass the flag on.
No GPU."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from stem_kernel_amd import _lib
from tests import svm_ref, svm_shrink_ref
from tests.svm_ref import BAD, as_problem, bits, hexes, one_class_lists
from tests.svm_shrink_ref import assert_is_the_record, assert_same

PROBLEMS, GRAMS = svm_shrink_ref.fixture()
IDS = [p["name"] for p in PROBLEMS]
OFF_PROBLEMS, _ = svm_ref.fixture()


@pytest.mark.parametrize("p", PROBLEMS, ids=IDS)
def test_host_path_equals_the_reference_solver_with_shrinking(p):
    K, y = GRAMS[p["gram"]]
    s = ska.svm_train_batch(K, y, [as_problem(p)], shrinking=True)[0]
    assert_is_the_record(s, p)
    alpha = hexes(p["alpha"])
    Cs = np.where(y[np.asarray(p["train"])] > 0, p["Cp"], p["Cn"])
    assert s.n_bound == int((alpha >= Cs).sum()) and s.n_free == int(((alpha > 0) & (alpha < Cs)).sum())


def test_fixture_covers_what_it_must():
    info = [p["info"] for p in PROBLEMS]
    ls = [len(p["train"]) for p in PROBLEMS]
    assert sum(4 * i["min_active"] < l for i, l in zip(info, ls)) >= 5
    assert sum(i["unshrunk"] for i in info) >= 3
    assert sum(i["regrown"] for i in info) >= 1
    assert sum(i["resumed"] > 0 for i in info) >= 2
    assert sum(p["status"] == 1 and 0 < p["capped_active"] < len(p["train"]) for p in PROBLEMS) >= 1
    # with shrinking the reference ends elsewhere (the generator asserts the same five)
    off = {p["name"]: p for p in OFF_PROBLEMS}
    assert sum(p["alpha"] != off[p["name"]]["alpha"] for p in PROBLEMS if p["name"] in off) >= 5


@pytest.mark.parametrize("name", ["l = 2", "int300 C=0.125", "int300 Cp != Cn"])
def test_a_run_without_a_shrink_call_is_the_run_without_shrinking(name):
    p = next(p for p in PROBLEMS if p["name"] == name)
    q = next(q for q in OFF_PROBLEMS if q["name"] == name)
    K, y = GRAMS[p["gram"]]
    s = ska.svm_train_batch(K, y, [as_problem(p)], shrinking=True)[0]
    assert s.shrink == dict(shrink_calls=0, shrunk_calls=0, min_active=len(p["train"]), unshrunk=0, regrown=0,
                            reconstructions=0, resumed=0)
    assert np.array_equal(bits(s.alpha), bits(hexes(q["alpha"])))
    assert (s.rho, s.obj, s.iterations) == (float.fromhex(q["rho"]), float.fromhex(q["obj"]), q["iterations"])


def old_host_call(K, y, ps, n_threads=0):
    """sk_svm_train_batch_host itself (the entry point without the flag):
    (alpha, dec, solutions) with the outputs concatenated in problem order."""
    K = np.ascontiguousarray(K, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    lists = [(np.ascontiguousarray(p["train"], dtype=np.int32), np.ascontiguousarray(p.get("test", []), dtype=np.int32))
             for p in ps]
    arr = (_lib.SvmProblem * len(ps))()
    for a, p, (tr, ts) in zip(arr, ps, lists):
        a.train, a.n_train = tr.ctypes.data_as(_lib._I32P), len(tr)
        a.test, a.n_test = (ts.ctypes.data_as(_lib._I32P) if len(ts) else None), len(ts)
        a.Cp, a.Cn, a.eps, a.max_iter = p["Cp"], p["Cn"], p["eps"], p["max_iter"]
    alpha = np.zeros(sum(len(tr) for tr, _ in lists))
    dec = np.zeros(max(sum(len(ts) for _, ts in lists), 1))
    sol = (_lib.SvmSolution * len(ps))()
    _lib.check(_lib.lib().sk_svm_train_batch_host(
        K.ctypes.data_as(_lib._F64P), len(y), y.ctypes.data_as(_lib._F64P), arr, len(ps), n_threads,
        alpha.ctypes.data_as(_lib._F64P), dec.ctypes.data_as(_lib._F64P), sol))
    return alpha, dec, sol


def test_flag_off_is_the_call_without_the_flag():
    K, y = GRAMS[0]
    ps = [dict(as_problem(p), test=[(3 * k + j) % 300 for j in range(4)])
          for k, p in enumerate(OFF_PROBLEMS) if p["gram"] == 0 and p["iterations"] < 6000]
    assert len(ps) >= 10
    alpha, dec, sol = old_host_call(K, y, ps)
    got = ska.svm_train_batch(K, y, ps, shrinking=False)
    assert np.array_equal(bits(np.concatenate([s.alpha for s in got])), bits(alpha))
    assert np.array_equal(bits(np.concatenate([s.decision for s in got])), bits(dec))
    for s, o, p in zip(got, sol, ps):
        assert (s.rho, s.obj, s.iterations, s.n_free, s.n_bound) == (o.rho, o.obj, o.iterations, o.n_free, o.n_bound)
        assert s.status == ska.svm.STATUS[o.status]
        assert s.shrink == dict(shrink_calls=0, shrunk_calls=0, min_active=len(p["train"]), unshrunk=0, regrown=0,
                                reconstructions=0, resumed=0)
    # info may be NULL
    n = len(ps[0]["train"])
    a, s1 = np.zeros(n), (_lib.SvmSolution * 1)()
    arr = (_lib.SvmProblem * 1)()
    tr = np.ascontiguousarray(ps[0]["train"], dtype=np.int32)
    arr[0].train, arr[0].n_train, arr[0].test, arr[0].n_test = tr.ctypes.data_as(_lib._I32P), n, None, 0
    arr[0].Cp, arr[0].Cn, arr[0].eps, arr[0].max_iter = ps[0]["Cp"], ps[0]["Cn"], ps[0]["eps"], ps[0]["max_iter"]
    Kc, yc = np.ascontiguousarray(K), np.ascontiguousarray(y)
    for flag in (0, 1):
        _lib.check(_lib.lib().sk_svm_train_batch_host_ex(
            Kc.ctypes.data_as(_lib._F64P), len(y), yc.ctypes.data_as(_lib._F64P), arr, 1, 1, flag,
            a.ctypes.data_as(_lib._F64P), None, s1, None))
        want = ska.svm_train_batch(K, y, [dict(ps[0], test=None)], shrinking=bool(flag))[0]
        assert np.array_equal(bits(a), bits(want.alpha)) and s1[0].rho == want.rho


def test_batch_equals_each_problem_alone_in_any_order():
    K, y = GRAMS[0]
    ps = [as_problem(p) for p in PROBLEMS if p["gram"] == 0 and p["iterations"] < 6000]
    assert len(ps) >= 10
    for k, p in enumerate(ps):
        p["test"] = [(7 * k + j) % 300 for j in range(5)]
    alone = [ska.svm_train_batch(K, y, [p], shrinking=True)[0] for p in ps]
    n = len(ps)
    for order in (list(range(n)), list(reversed(range(n))), sorted(range(n), key=lambda k: (5 * k + 3) % 7)):
        got = ska.svm_train_batch(K, y, [ps[k] for k in order], n_threads=3, shrinking=True)
        for k, s in zip(order, got):
            assert_same(s, alone[k], k)
            assert np.array_equal(bits(s.decision), bits(alone[k].decision))


def test_decision_values_are_the_sequential_sum_in_training_order():
    p = next(p for p in PROBLEMS if p["name"] == "partial list")
    K, y = GRAMS[p["gram"]]
    test = list(range(0, 300, 7))
    s = ska.svm_train_batch(K, y, [dict(as_problem(p), test=test)], shrinking=True)[0]
    assert_is_the_record(s, p)
    ys = np.where(y[p["train"]] > 0, 1.0, -1.0)
    for q, t in enumerate(test):
        acc = 0.0
        for a in range(len(p["train"])):
            if s.alpha[a] != 0.0:
                acc += s.alpha[a] * ys[a] * K[t, p["train"][a]]
        assert s.decision[q] == acc - s.rho


@pytest.mark.parametrize("name", list(BAD) + ["positives only", "negatives only"])
def test_invalid_arguments_are_refused(name):
    K, y = GRAMS[0]
    bad = {**BAD, **one_class_lists(y)}[name]
    good = dict(train=[0, 1, 2])
    for batch in ([bad], [good, bad]):  # alone, and after a valid problem
        with pytest.raises(ska.StemKernelError) as e:
            ska.svm_train_batch(K, y, batch, shrinking=True)
        assert e.value.code == -1


def test_iteration_cap_ends_like_an_optimum():
    """max_iter met exactly is still "converged"; one short is the capped state."""
    p = next(p for p in PROBLEMS if p["name"] == "l = 3")
    K, y = GRAMS[p["gram"]]
    for cap in (p["iterations"], p["iterations"] + 1):
        assert_is_the_record(ska.svm_train(K, y, train=p["train"], C=p["Cp"], max_iter=cap, shrinking=True), p)
    t = ska.svm_train(K, y, train=p["train"], C=p["Cp"], max_iter=p["iterations"] - 1, shrinking=True)
    assert t.status == "not converged" and t.iterations == p["iterations"] - 1


def test_cross_validate_and_auc_objective_pass_the_flag_on():
    K, y = GRAMS[0]
    folds = [next(p for p in PROBLEMS if p["name"] == f"split ncv=5 cv={f}") for f in range(5)]
    cv = ska.cross_validate(K, y, 5, [1.0], shrinking=True)
    cv_off = ska.cross_validate(K, y, 5, [1.0])
    f, g, records = ska.auc_objective(K, None, y, 5, 1.0, shrinking=True)
    f_off, g_off, records_off = ska.auc_objective(K, None, y, 5, 1.0)
    for k, p in enumerate(folds):
        assert_is_the_record(cv.solutions[0][k], p)
        assert_is_the_record(records[k]["solution"], p)
        off = next(q for q in OFF_PROBLEMS if q["name"] == p["name"])
        for s in (cv_off.solutions[0][k], records_off[k]["solution"]):
            assert np.array_equal(bits(s.alpha), bits(hexes(off["alpha"]))) and s.shrink["shrink_calls"] == 0
        # the gradient is taken on those alphas
        r = ska.auc_gradient_batch(K, None, y, [dict(train=p["train"], test=svm_ref.split(300, 5, k)[1], C=1.0,
                                                     alpha=hexes(p["alpha"]), rho=float.fromhex(p["rho"]),
                                                     delta=records[k]["delta"])])[0]
        assert r.cg == records[k]["gradient"].cg
    acc = 0.0
    for r in records:  # Optimizer::optimize: g[0] -= cg in fold order
        acc -= r["gradient"].cg
    assert g[0] == acc
    assert (f, g[0]) != (f_off, g_off[0])
