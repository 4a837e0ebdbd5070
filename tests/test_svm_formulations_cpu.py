"""nu-SVC, one-class, epsilon-SVR and nu-SVR training, host path
(sk_svm_solve_batch_host): pinned to the reference's own solve_nu_svc,
solve_one_class, solve_epsilon_svr and solve_nu_svr through
tests/golden/svm_formulations.json (made by
tools/make_golden_svm_formulations.py from libsvm/svm.cpp, solver.cpp and
qmatrix.cpp compiled in place, run without shrinking); C-SVC through the new
call against sk_svm_train_batch; batching, decision values, the refusals, the
model round trip and KKT sanity.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import stem_kernel_amd as ska
from tests import svm_formulations_ref as fr
from tests import svm_ref
from tests.svm_formulations_ref import as_task, bits, f64, hexes, same_bits, targets_of

PROBLEMS, GRAMS = fr.fixture()
IDS = [p["name"] for p in PROBLEMS]
BY_NAME = {p["name"]: p for p in PROBLEMS}


def solve(p, **more):
    g = GRAMS[p["gram"]]
    return ska.svm_train_batch(g[0], targets_of(p, g), [as_task(p, **more)])[0]


@pytest.mark.parametrize("p", PROBLEMS, ids=IDS)
def test_host_path_equals_the_reference(p):
    s = solve(p)
    coef = hexes(p["coef"])
    assert s.svm_type == p["svm_type"]
    assert np.array_equal(bits(s.coef), bits(coef)), np.flatnonzero(bits(s.coef) != bits(coef))[:8]
    assert same_bits(s.rho, f64(p["rho"])) and same_bits(s.obj, f64(p["obj"])) and same_bits(s.r, f64(p["r"])), \
        (s.rho, p["rho"], s.obj, p["obj"], s.r, p["r"])
    assert s.iterations == p["iterations"]
    assert s.status == ("not converged" if p["status"] else "converged")
    assert (s.n_bound, s.n_free) == (p["n_bound"], p["n_free"])


def test_fixture_covers_what_it_must():
    for ty in fr.TYPES:
        ps = [p for p in PROBLEMS if p["svm_type"] == ty]
        names = " ".join(p["name"] for p in ps)
        ls = [len(p["train"]) for p in ps]
        assert min(ls) == 2 and max(ls) == 300
        assert sum(len(p["train"]) == 300 and p["max_iter"] > 7 for p in ps) >= 2
        for need in ("TAU", "rbf l = 40", "indefinite", "permuted partial", "max_iter 7"):
            assert need in names, (ty, need)
        assert any(p["max_iter"] == 7 and p["status"] == 1 and p["iterations"] == 7 for p in ps)
        assert all(p["iterations"] < 40_000 for p in ps)
    K, y, _ = GRAMS[2]
    assert np.array_equal(K[0], K[1])  # the identical pair: quad_coef is 0
    assert np.linalg.eigvalsh(GRAMS[1][0]).min() < -1.0
    for g in GRAMS:
        assert np.array_equal(g[2] * 4, np.round(g[2] * 4)) and np.abs(g[2]).max() <= 8  # multiples of 1/4
    # nu-SVC: nu l / 2 integer, fractional, and equal to min(n+, n-)
    p = BY_NAME["nu_svc: nu l / 2 integer"]
    assert p["nu"] * 300 / 2 == 75.0
    p = BY_NAME["nu_svc: nu l / 2 fractional"]
    assert p["nu"] * 300 / 2 != round(p["nu"] * 300 / 2)
    p = BY_NAME["nu_svc: nu l / 2 == min(n+, n-)"]
    yy = GRAMS[p["gram"]][1][p["train"]]
    assert p["nu"] * len(yy) / 2 == min((yy > 0).sum(), (yy <= 0).sum()) == 24
    # one-class: every alpha at the bound at nu = 1; a fractional remainder
    p = BY_NAME["one_class: nu = 1"]
    assert int(p["nu"] * len(p["train"])) == len(p["train"]) and all(f64(c) == 1.0 for c in p["coef"])
    p = BY_NAME["one_class: fractional nu l"]
    assert p["nu"] * 40 != int(p["nu"] * 40)
    # nu-SVR: C nu l / 2 runs out partway through the list
    p = BY_NAME["nu_svr: start point runs out"]
    assert 0 < p["C"] * p["nu"] * 300 / 2 / p["C"] < 299
    # epsilon-SVR: p = 0, and p over every |target| leaves every coefficient zero
    assert BY_NAME["epsilon_svr: p = 0"]["p"] == 0.0
    p = BY_NAME["epsilon_svr: p over every |target|"]
    assert p["p"] > np.abs(GRAMS[p["gram"]][2]).max() and all(f64(c) == 0.0 for c in p["coef"])


def test_c_svc_through_the_new_call_is_sk_svm_train_batch():
    P0, G0 = svm_ref.fixture()
    for name in ("int300 C=1", "permuted list", "max_iter 7", "rbf C=64", "identical pair, l = 2 (TAU)"):
        p = next(q for q in P0 if q["name"] == name)
        K, y = G0[p["gram"]]
        test = list(range(0, len(y), 3))
        old = ska.svm_train_batch(K, y, [dict(svm_ref.as_problem(p), test=test)])[0]
        new = ska.svm_train_batch(K, y, [dict(train=p["train"], test=test, C=p["Cp"], eps=p["eps"],
                                              max_iter=p["max_iter"], svm_type="c_svc")])[0]
        assert np.array_equal(bits(new.alpha), bits(old.alpha))
        ys = np.where(y[np.asarray(p["train"])] > 0, 1.0, -1.0)
        assert np.array_equal(bits(new.coef), bits(old.alpha * ys)) and np.array_equal(bits(old.coef), bits(new.coef))
        assert (new.rho, new.obj, new.iterations, new.status, new.n_free, new.n_bound, new.r) == \
            (old.rho, old.obj, old.iterations, old.status, old.n_free, old.n_bound, 0.0)
        assert np.array_equal(bits(new.decision), bits(old.decision))
        assert np.array_equal(bits(new.alpha), bits(hexes(p["alpha"])))


def mixed_batch():
    """Tasks of all five types over the 300-example Gram: (targets per task, tasks)."""
    K, y, t = GRAMS[0]
    ps = [p for p in PROBLEMS if p["gram"] == 0]
    tasks = [as_task(p, test=[(7 * k + j) % 300 for j in range(5)]) for k, p in enumerate(ps)]
    tasks.append(dict(train=list(range(0, 300, 2)), test=[1, 3], C=0.5, svm_type="c_svc", max_iter=fr.CAP))
    return K, y, t, ps, tasks


def test_mixed_batch_equals_each_task_alone_in_any_order():
    """Classifier labels and SVR targets are one array per call, so the mixed
    batch runs on targets whose signs are the class labels: sign(y) * (|t| + 1)."""
    K, y, t, ps, tasks = mixed_batch()
    both = y * (np.abs(t) + 1.0)
    assert len(tasks) >= 25 and {q["svm_type"] for q in tasks} == {"c_svc", *fr.TYPES}
    alone = [ska.svm_train_batch(K, both, [q])[0] for q in tasks]
    n = len(tasks)
    shuffled = sorted(range(n), key=lambda k: (k * 7919 + 13) % 1009)
    assert sorted(shuffled) == list(range(n))
    for order in (list(range(n)), list(reversed(range(n))), shuffled):
        got = ska.svm_train_batch(K, both, [tasks[k] for k in order], n_threads=3)
        for k, s in zip(order, got):
            fr.assert_same_solution(s, alone[k], tasks[k]["svm_type"])
            assert np.array_equal(bits(s.decision), bits(alone[k].decision))
    # the classifiers and one-class do not read the magnitudes: the fixture's bits
    for p, s in zip(ps, alone):
        if p["svm_type"] in ("nu_svc", "one_class"):
            assert np.array_equal(bits(s.coef), bits(hexes(p["coef"]))), p["name"]
    # the c_svc task, solved among the other four types, is its problem through the untyped call
    q = tasks[-1]
    assert q["svm_type"] == "c_svc"
    new = got[order.index(n - 1)]
    old = ska.svm_train_batch(K, both, [dict(train=q["train"], test=q["test"], C=q["C"], max_iter=q["max_iter"])])[0]
    assert np.array_equal(bits(new.alpha), bits(old.alpha)) and np.array_equal(bits(new.coef), bits(old.coef))
    assert np.array_equal(bits(new.decision), bits(old.decision))
    assert (new.rho, new.obj, new.iterations, new.status, new.n_free, new.n_bound, new.r) == \
        (old.rho, old.obj, old.iterations, old.status, old.n_free, old.n_bound, 0.0)


@pytest.mark.parametrize("name", ["nu_svc: rbf l = 40", "one_class: rbf l = 40", "epsilon_svr: rbf l = 40",
                                  "nu_svr: rbf l = 40", "nu_svr: permuted partial list"])
def test_decision_values_are_the_sequential_sum(name):
    p = BY_NAME[name]
    K = GRAMS[p["gram"]][0]
    test = list(range(1, len(K), 2))
    s = solve(p, test=test)
    assert np.count_nonzero(s.coef) >= 2
    for q, t in enumerate(test):
        acc = 0.0
        for a, ta in enumerate(p["train"]):
            if s.coef[a] != 0.0:
                acc += s.coef[a] * K[t, ta]
        assert s.decision[q] == acc - s.rho


BAD = fr.bad_tasks(GRAMS[0][1])


@pytest.mark.parametrize("name", list(BAD))
def test_invalid_tasks_are_refused(name):
    K, y, t = GRAMS[0]
    good = dict(svm_type="one_class", train=[0, 1, 2])
    for batch in ([BAD[name]], [good, BAD[name]]):
        with pytest.raises(ska.StemKernelError) as e:
            ska.svm_train_batch(K, y, batch)
        assert e.value.code == -1, name


def test_unknown_svm_type_is_refused_by_the_c_entry_point():
    """The Python layer knows the five names only; the integers outside 0 .. 4
    reach sk_svm_solve_batch_host through ctypes."""
    import ctypes as C
    from stem_kernel_amd import _lib
    K, y, _ = GRAMS[0]
    train = np.array([0, 1, 2, 3], dtype=np.int32)
    coef, sol = np.zeros(4), (_lib.SvmTaskSolution * 1)()
    for ty, want in ((-1, -1), (5, -1), (2, 0)):
        task = (_lib.SvmTask * 1)()
        task[0].train, task[0].n_train, task[0].n_test = train.ctypes.data_as(_lib._I32P), 4, 0
        task[0].svm_type, task[0].C, task[0].nu, task[0].p, task[0].eps, task[0].max_iter = ty, 1.0, 0.5, 0.1, 1e-3, 1000
        rc = ska.lib().sk_svm_solve_batch_host(K.ctypes.data_as(_lib._F64P), len(y), y.ctypes.data_as(_lib._F64P), task,
                                               1, 1, coef.ctypes.data_as(_lib._F64P), None, sol)
        assert rc == want, (ty, rc)
    with pytest.raises(ValueError, match="svm_type 'c_svr'"):
        ska.svm_train_batch(K, y, [dict(svm_type="c_svr")], shrinking=True)  # unknown, not "no shrinking"


def test_targets_that_are_not_finite_are_refused_for_svr_only():
    K, y, t = GRAMS[0]
    for name, (bad_t, task) in fr.bad_targets(t).items():
        with pytest.raises(ska.StemKernelError) as e:
            ska.svm_train_batch(K, bad_t, [task])
        assert e.value.code == -1, name
        # outside the training list, or for one-class, the value is not read
        ska.svm_train_batch(K, bad_t, [dict(task, train=[0, 1, 3]), dict(svm_type="one_class", train=[0, 1, 2])])


def test_feasibility_edge_and_python_refusals():
    K, y, t = GRAMS[0]
    s = ska.svm_train_batch(K, y, [fr.feasible_edge(y)])[0]  # nu l / 2 == min(n+, n-): the check is >
    assert s.status == "converged"
    with pytest.raises(ValueError, match="shrinking"):
        ska.svm_train_batch(K, y, [dict(svm_type="nu_svc", nu=0.2)], shrinking=True)
    with pytest.raises(ValueError, match="shrinking"):
        ska.svm_train(K, t, svm_type="epsilon_svr", shrinking=True)
    with pytest.raises(ValueError, match="svm_type"):
        ska.svm_train_batch(K, y, [dict(svm_type="c_svr")])
    with pytest.raises(ValueError, match="every problem"):
        ska.svm_train_batch(K, y, [dict(svm_type="one_class"), dict(C=1.0)])
    # c_svc with shrinking keeps working when it is named
    a = ska.svm_train(K, y, C=0.5, svm_type="c_svc", shrinking=True, train=np.arange(100))
    b = ska.svm_train(K, y, C=0.5, shrinking=True, train=np.arange(100))
    assert np.array_equal(bits(a.alpha), bits(b.alpha)) and a.shrink == b.shrink
    # svm_train with a type is svm_train_batch with one task
    p = BY_NAME["nu_svr: rbf l = 40"]
    g = GRAMS[p["gram"]]
    s = ska.svm_train(g[0], g[2], C=p["C"], svm_type="nu_svr", nu=p["nu"], train=p["train"], eps=p["eps"])
    assert np.array_equal(bits(s.coef), bits(hexes(p["coef"]))) and s.r == f64(p["r"])
    shape, base = ska.svm_solve_shape(), ska.svm_train_shape()["max_train"]
    assert shape == {"c_svc": base, "nu_svc": base, "one_class": base, "epsilon_svr": base // 2,
                     "nu_svr": base // 2}


def test_host_path_takes_any_length():
    K, y, t = GRAMS[0]
    train = [k % 300 for k in range(ska.svm_solve_shape()["epsilon_svr"] + 1)]
    s = ska.svm_train(K, t, train=train, C=2.0 ** -6, svm_type="epsilon_svr", max_iter=500)
    assert len(s.coef) == len(train) and s.iterations >= 1


ROUND_TRIP = ["nu_svc: rbf l = 40", "nu_svc: permuted partial list", "one_class: rbf l = 40",
              "one_class: int300 nu=0.5", "epsilon_svr: rbf l = 40", "epsilon_svr: permuted partial list",
              "nu_svr: rbf l = 40", "nu_svr: int300 C=2 nu=0.25"]


@pytest.mark.parametrize("name", ["c_svc"] + ROUND_TRIP)
def test_written_model_predicts_the_batch_decision_values(name, tmp_path):
    """save(), sk_svm_model_load, sk_svm_predict of every example's Gram row:
    the solution's decision value within 2 l 2^-53 sum |term| (the model
    stores coefficients as %.16g and rho as %g)."""
    if name == "c_svc":
        K, y, t = GRAMS[3]
        task = dict(train=list(range(40)), C=8.0, svm_type="c_svc")
        tg = y
    else:
        p = BY_NAME[name]
        K, y, t = GRAMS[p["gram"]]
        task, tg = as_task(p), targets_of(p, GRAMS[p["gram"]])
    n = len(y)
    train = np.asarray(task["train"])
    s = ska.svm_train_batch(K, tg, [dict(task, test=list(range(n)))])[0]
    m = s.model(str(tmp_path / "m.model"))
    ty = ska.svm.SVM_TYPES[s.svm_type]
    assert m.svm_type == ty and m.nr_class == 2
    text = (tmp_path / "m.model").read_text().split("\n")
    assert text[0] == f"svm_type {s.svm_type}" and text[1] == "kernel_type precomputed"
    sgn = 1.0
    if ty in (0, 1):
        first = y[train[0]]
        assert m.labels == [int(first), int(-first)]
        sgn = 1.0 if first > 0 else -1.0  # libsvm's +1 is its first class
        assert text[5].startswith("label ") and text[6].startswith("nr_sv ") and text[7] == "SV"
    else:
        # svm.cpp:677-717: no label and nr_sv lines, SVs in list order
        assert text[2:4] == ["nr_class 2", f"total_sv {np.count_nonzero(s.coef)}"] and text[5] == "SV"
        assert [int(v.split("0:")[1]) for v in text[6:-1]] == [int(k) + 1 for k in train[s.coef != 0]]
    rho_printed = float("%g" % (sgn * s.rho))
    assert np.count_nonzero(s.coef) >= 2
    for q in range(n):
        label, vals = m.predict(K[q], cnt=q + 1, probability=False)
        terms = s.coef * K[q, train]
        bound = 2 * len(terms) * 2.0 ** -53 * (np.abs(terms).sum() + abs(s.rho))
        want = sgn * (s.decision[q] + s.rho) - rho_printed
        assert abs(vals[0] - want) <= bound, (q, vals[0], want, bound)
        if ty == 2 and abs(want) > bound:
            assert label == (1.0 if want > 0 else -1.0)  # one-class: the sign of the value
        if ty in (3, 4):
            assert label == vals[0]


def test_model_text_is_svm_save_model_layout(tmp_path):
    sol = ska.SVMSolution.__new__(ska.SVMSolution)
    sol.labels, sol.train = np.array([0.5, -1.25, 3.0, 0.0]), np.array([2, 0, 3, 1], dtype=np.int32)
    sol.alpha, sol.coef, sol.rho, sol.svm_type = None, np.array([0.5, 0.0, -1.0 / 3.0, -0.0]), -0.123456789, "nu_svr"
    sol.save(str(tmp_path / "a.model"))
    assert (tmp_path / "a.model").read_text().split("\n") == [
        "svm_type nu_svr", "kernel_type precomputed", "nr_class 2", "total_sv 2", "rho -0.123457", "SV",
        "0.5 0:3 ", "-0.3333333333333333 0:4 ", ""]
    sol.svm_type = "one_class"
    sol.save(str(tmp_path / "b.model"))
    assert (tmp_path / "b.model").read_text().split("\n")[0] == "svm_type one_class"
    # nu-SVC: the classifier layout; the first training label is negative, so signs turn
    sol.labels, sol.svm_type = np.array([1.0, -1.0, -1.0, 1.0]), "nu_svc"
    sol.coef = np.array([-0.25, 2.0, 0.0, -1e-5])
    sol.save(str(tmp_path / "c.model"))
    assert (tmp_path / "c.model").read_text().split("\n") == [
        "svm_type nu_svc", "kernel_type precomputed", "nr_class 2", "total_sv 3", "rho 0.123457", "label -1 1",
        "nr_sv 2 1", "SV", "0.25 0:3 ", "1e-05 0:2 ", "-2 0:1 ", ""]


def test_kkt_sanity_on_the_l300_problems():
    """Independent of the fixture: the constraints each formulation keeps."""
    K, y, t = GRAMS[0]
    for p in PROBLEMS:
        if p["gram"] != 0 or len(p["train"]) != 300 or p["max_iter"] == 7:
            continue
        s = solve(p)
        l, ty = 300, p["svm_type"]
        ys = np.where(y[np.asarray(p["train"])] > 0, 1.0, -1.0)
        tol = 300 * 2.0 ** -50
        if ty == "nu_svc":
            # sum over each class of alpha = nu l / 2, and coef = alpha y / r
            a = s.coef * ys * s.r
            assert np.all(a >= 0) and np.all(a <= 1 + tol)
            for side in (ys > 0, ys < 0):
                assert abs(a[side].sum() - p["nu"] * l / 2) <= tol * p["nu"] * l, p["name"]
            assert abs(s.coef.sum()) <= tol * np.abs(s.coef).sum()
        elif ty == "one_class":
            assert np.all(s.coef >= 0) and np.all(s.coef <= 1)
            assert abs(s.coef.sum() - p["nu"] * l) <= tol * p["nu"] * l, p["name"]
        else:
            assert np.all(np.abs(s.coef) <= p["C"]), p["name"]
            assert abs(s.coef.sum()) <= tol * max(np.abs(s.coef).sum(), 1.0), p["name"]  # y^T alpha = 0


def test_host_code_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/svm_formulations_sanitize.cpp with csrc/host/svm_train.cpp,
    built with -fsanitize=address,undefined as a stand-alone program."""
    src = os.path.join(svm_ref.ROOT, "tests", "cpp", "svm_formulations_sanitize.cpp")
    host = os.path.join(svm_ref.ROOT, "stem_kernel_amd", "csrc", "host", "svm_train.cpp")
    exe = str(tmp_path / "svm_formulations_sanitize")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(svm_ref.ROOT, "include"), src, host,
                    "-pthread", "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok: 5 types" in out.stdout
    # the C-SVC part met what it is there for: a stop at max_iter with shrinking off and on, problems
    # that shrank, and one whose unshrink branch regrew the active set
    seen = re.search(r"^c_svc: capped (\d+) shrunk (\d+) regrown (\d+)$", out.stdout, re.M)
    assert seen, out.stdout
    capped, shrunk, regrown = map(int, seen.groups())
    assert capped == 2 and shrunk >= 2 and regrown >= 1, out.stdout
