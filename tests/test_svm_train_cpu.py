"""C-SVC training, host path (sk_svm_train_batch_host): pinned to the
reference's own SMO solver through tests/golden/svm_train.json (made by
tools/make_golden_svm_train.py from libsvm/solver.cpp compiled in place, run
without shrinking); batching, the iteration cap, the error codes, the
cross-validation split and the model writer.  No GPU."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from tests import svm_ref

from tests.svm_ref import BAD, as_problem, bits, hexes, one_class_lists

PROBLEMS, GRAMS = svm_ref.fixture()
IDS = [p["name"] for p in PROBLEMS]


@pytest.mark.parametrize("p", PROBLEMS, ids=IDS)
def test_host_path_equals_the_reference_solver(p):
    K, y = GRAMS[p["gram"]]
    s = ska.svm_train_batch(K, y, [as_problem(p)])[0]
    alpha = hexes(p["alpha"])
    assert np.array_equal(bits(s.alpha), bits(alpha)), np.flatnonzero(bits(s.alpha) != bits(alpha))[:8]
    # rho and obj: within l 2^-52 sum |term| of the recorded values -- and, the
    # sums being added in the reference's order, the recorded bits themselves
    l = len(p["train"])
    rho_b, obj_b = svm_ref.sum_bounds(K, y, p["train"], p["Cp"], p["Cn"], alpha, l * 2.0 ** -52)
    rho, obj = float.fromhex(p["rho"]), float.fromhex(p["obj"])
    print(f"{p['name']}: rho {s.rho!r} ref {rho!r} bound {rho_b:.3g}; obj {s.obj!r} ref {obj!r} bound {obj_b:.3g}")
    assert abs(s.rho - rho) <= rho_b
    assert abs(s.obj - obj) <= obj_b
    assert s.rho == rho and s.obj == obj
    assert s.iterations == p["iterations"]
    assert s.status == ("not converged" if p["status"] else "converged")
    C = np.where(y[np.asarray(p["train"])] > 0, p["Cp"], p["Cn"])
    assert s.n_bound == int((alpha >= C).sum()) and s.n_free == int(((alpha > 0) & (alpha < C)).sum())


def test_fixture_covers_what_it_must():
    names = " ".join(IDS)
    ls = [len(p["train"]) for p in PROBLEMS]
    assert min(ls) == 2 and max(ls) >= 300
    assert {0.125, 1.0, 64.0} <= {p["Cp"] for p in PROBLEMS}
    assert any(p["Cp"] != p["Cn"] for p in PROBLEMS)
    assert any(p["max_iter"] == 7 and p["status"] == 1 for p in PROBLEMS)
    for need in ("permuted", "partial", "TAU", "indefinite", "split ncv=5 cv=4", "rbf"):
        assert need in names
    # the identical pair: equal rows of K, opposite labels, so quad_coef is 0
    K, y = GRAMS[2]
    assert np.array_equal(K[0], K[1]) and y[0] == -y[1]
    # the indefinite Gram has a negative eigenvalue
    assert np.linalg.eigvalsh(GRAMS[1][0]).min() < -1.0


def test_batch_equals_each_problem_alone_in_any_order():
    K, y = GRAMS[0]
    ps = [as_problem(p) for p in PROBLEMS if p["gram"] == 0 and p["iterations"] < 6000]
    assert len(ps) >= 10
    for k, p in enumerate(ps):
        p["test"] = [(7 * k + j) % 300 for j in range(5)]
    alone = [ska.svm_train_batch(K, y, [p])[0] for p in ps]
    for order in (list(range(len(ps))), list(reversed(range(len(ps)))), [3, 0, 7, 1, 5, 2, 6, 4, 9, 8]):
        got = ska.svm_train_batch(K, y, [ps[k] for k in order], n_threads=3)
        for k, s in zip(order, got):
            a = alone[k]
            assert np.array_equal(bits(s.alpha), bits(a.alpha))
            assert np.array_equal(bits(s.decision), bits(a.decision))
            assert (s.rho, s.obj, s.iterations, s.status, s.n_free, s.n_bound) == \
                (a.rho, a.obj, a.iterations, a.status, a.n_free, a.n_bound)


def test_iteration_cap_is_reported_not_raised():
    p = next(p for p in PROBLEMS if p["max_iter"] == 7)
    K, y = GRAMS[p["gram"]]
    s = ska.svm_train(K, y, train=p["train"], Cp=p["Cp"], Cn=p["Cn"], eps=p["eps"], max_iter=7)
    assert s.status == "not converged" and not s.converged and s.iterations == 7
    # a cap the problem does not reach changes nothing; a cap met exactly is still "converged"
    q = next(q for q in PROBLEMS if q["name"] == "l = 3")
    for cap in (q["iterations"], q["iterations"] + 1):
        t = ska.svm_train(K, y, train=q["train"], C=q["Cp"], eps=q["eps"], max_iter=cap)
        assert t.status == "converged" and t.iterations == q["iterations"]
        assert np.array_equal(bits(t.alpha), bits(hexes(q["alpha"])))
    t = ska.svm_train(K, y, train=q["train"], C=q["Cp"], eps=q["eps"], max_iter=q["iterations"] - 1)
    assert t.status == "not converged" and t.iterations == q["iterations"] - 1
    assert ska.DEFAULT_MAX_ITER >= 1_000_000


@pytest.mark.parametrize("name", list(BAD) + ["positives only", "negatives only"])
def test_invalid_arguments_are_refused(name):
    K, y = GRAMS[0]
    bad = {**BAD, **one_class_lists(y)}[name]
    good = dict(train=[0, 1, 2])
    for batch in ([bad], [good, bad]):  # alone, and after a valid problem
        with pytest.raises(ska.StemKernelError) as e:
            ska.svm_train_batch(K, y, batch)
        assert e.value.code == -1


def test_host_path_takes_any_length():
    # beyond the GPU solver's largest class: repeated examples, so the Gram stays small
    K, y = GRAMS[0]
    train = [k % 300 for k in range(ska.svm_train_shape()["max_train"] + 1)]
    s = ska.svm_train(K, y, train=train, C=2.0 ** -6, max_iter=2000)
    assert len(s.alpha) == len(train) and s.iterations >= 1


def test_cross_validation_uses_the_reference_split():
    K, y = GRAMS[0]
    n, ncv = len(y), 5
    cv = ska.cross_validate(K, y, ncv, [0.125, 1.0], eps=1e-3)
    for f, (tr, ts) in enumerate(cv.folds):
        # Optimizer::split (optimizer/optimizer.cpp:99-116), restated as its loop
        tr_i, ts_i = [], []
        for j in range(n):
            (tr_i if j % ncv != f else ts_i).append(j)
        assert tr.tolist() == tr_i and ts.tolist() == ts_i
        assert tr.tolist() == svm_ref.split(n, ncv, f)[0].tolist()
    # the C = 1 row is the fixture's five fold problems
    for f, s in enumerate(cv.solutions[1]):
        p = next(p for p in PROBLEMS if p["name"] == f"split ncv=5 cv={f}")
        assert np.array_equal(bits(s.alpha), bits(hexes(p["alpha"])))
        assert len(cv.decision[1][f]) == len(cv.folds[f][1])
    # accuracy and AUC from the decision values, recomputed here
    for c in range(2):
        dec = np.concatenate(cv.decision[c])
        lab = np.concatenate([y[ts] for _, ts in cv.folds])
        assert cv.accuracy[c] == pytest.approx(float(((dec > 0) == (lab > 0)).mean()), abs=1e-15)
        aucs = []
        for d, (_, ts) in zip(cv.decision[c], cv.folds):
            pos, neg = d[y[ts] > 0], d[y[ts] <= 0]
            aucs.append(np.mean([(a > b) + 0.5 * (a == b) for a in pos for b in neg]))
        assert cv.auc[c] == pytest.approx(float(np.mean(aucs)), abs=1e-12)
        assert 0.0 <= cv.auc[c] <= 1.0 and cv.converged[c]


def test_decision_values_are_the_sequential_sum():
    K, y = GRAMS[3]
    train, test = list(range(0, 40, 2)), list(range(1, 40, 2))
    s = ska.svm_train(K, y, C=8.0, train=train, test=test)
    ys = np.where(y[train] > 0, 1.0, -1.0)
    for q, t in enumerate(test):
        acc = 0.0
        for a in range(len(train)):
            if s.alpha[a] != 0.0:
                acc += s.alpha[a] * ys[a] * K[t, train[a]]
        assert s.decision[q] == acc - s.rho


@pytest.mark.parametrize("name", ["rbf C=64", "int300 Cp != Cn", "indefinite C=1", "permuted list"])
def test_written_model_predicts_the_batch_decision_values(name, tmp_path):
    p = next(p for p in PROBLEMS if p["name"] == name)
    K, y = GRAMS[p["gram"]]
    n = len(y)
    test = list(range(0, n, 3))
    s = ska.svm_train_batch(K, y, [dict(as_problem(p), test=test)])[0]
    m = s.model(str(tmp_path / "m.model"))
    assert m.svm_type == 0 and m.nr_class == 2
    first = y[p["train"][0]]
    assert m.labels == [int(first), int(-first)]  # svm_group_classes: by first appearance
    sgn = 1.0 if first > 0 else -1.0  # libsvm's +1 is its first class
    rho_printed = float("%g" % (sgn * s.rho))
    coef = s.alpha * np.where(y[np.asarray(p["train"])] > 0, 1.0, -1.0)
    for q, t in enumerate(test):
        label, vals = m.predict(K[t], cnt=t + 1, probability=False)
        terms = coef * K[t, np.asarray(p["train"])]
        bound = 2 * len(terms) * 2.0 ** -53 * (np.abs(terms).sum() + abs(s.rho))
        want = sgn * (s.decision[q] + s.rho) - rho_printed
        assert abs(vals[0] - want) <= bound, (t, vals[0], want, bound)
        if abs(want) > bound:
            assert label == (m.labels[0] if want > 0 else m.labels[1])


def test_model_text_is_svm_save_model_layout(tmp_path):
    # svm_save_model (libsvm/svm.cpp:1201-1286), line by line
    labels = np.array([1.0, -1.0, -1.0, 1.0, -1.0])
    sol = ska.SVMSolution.__new__(ska.SVMSolution)
    sol.labels, sol.train = labels, np.array([0, 1, 2, 3, 4], dtype=np.int32)
    sol.alpha, sol.rho = np.array([0.5, 0.0, 0.25, 0.75, 1.0 / 3.0]), 0.123456789
    sol.save(str(tmp_path / "a.model"))
    assert (tmp_path / "a.model").read_text().split("\n") == [
        "svm_type c_svc", "kernel_type precomputed", "nr_class 2", "total_sv 4", "rho 0.123457",
        "label 1 -1", "nr_sv 2 2", "SV", "0.5 0:1 ", "0.75 0:4 ", "-0.25 0:3 ", "-0.3333333333333333 0:5 ", ""]
    # first training label negative: libsvm's +1 class is -1, so signs flip; a permuted list
    sol.train = np.array([2, 4, 0, 3], dtype=np.int32)
    sol.alpha, sol.rho = np.array([0.25, 0.0, 1e-5, 2.0]), -1234567.0
    sol.save(str(tmp_path / "b.model"))
    assert (tmp_path / "b.model").read_text().split("\n") == [
        "svm_type c_svc", "kernel_type precomputed", "nr_class 2", "total_sv 3", "rho 1.23457e+06",
        "label -1 1", "nr_sv 1 2", "SV", "0.25 0:3 ", "-1e-05 0:1 ", "-2 0:4 ", ""]
    # one class, or a third label: refused
    for bad in (np.array([1.0, 1.0, 1.0, 1.0, 1.0]), np.array([1.0, -1.0, 2.0, 1.0, 3.0])):
        sol.labels = bad
        with pytest.raises(ska.StemKernelError):
            sol.save(str(tmp_path / "c.model"))
