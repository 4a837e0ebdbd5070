"""Inputs of the nu-SVC / one-class / epsilon-SVR / nu-SVR training tests
(tests/test_svm_formulations_cpu.py and tests/test_svm_formulations.py): the
fixture tests/golden/svm_formulations.json (the reference's own solve_*
functions, tools/make_golden_svm_formulations.py) with its Grams
materialised, the tasks as svm_train_batch takes them, the tasks
sk_svm_solve_batch refuses, and the size-class edge batches."""
import functools
import json
import os

import numpy as np

from tests import svm_ref
from tests.svm_ref import bits, hexes  # noqa: F401

FIXTURE = os.path.join(svm_ref.ROOT, "tests", "golden", "svm_formulations.json")
TYPES = ("nu_svc", "one_class", "epsilon_svr", "nu_svr")
SVR = ("epsilon_svr", "nu_svr")
CAP = 200_000


@functools.lru_cache(maxsize=None)
def fixture():
    """(problems, grams): grams[g] = (K, class labels, SVR targets)."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    grams = []
    for g in fx["grams"]:
        if g["kind"] == "int":
            K, y = svm_ref.int_gram(g["seed"], g["n"], g["d"], g["shift"], g["indef"], g["dup"])
            assert [int(v) for v in y] == g["labels"]
        else:
            n = g["n"]
            K = np.array([float.fromhex(v) for v in g["values"]]).reshape(n, n)
            y = np.array(g["labels"], dtype=np.float64)
        grams.append((K, y, np.array(g["targets"], dtype=np.float64)))
    return fx["problems"], grams


def targets_of(p, gram):
    """What sk_svm_solve_batch takes as targets for a task of p's type."""
    return gram[2] if p["svm_type"] in SVR else gram[1]


def as_task(p, **more):
    """A fixture record as svm_train_batch takes it, max_iter capped at CAP."""
    t = dict(train=p["train"], svm_type=p["svm_type"], C=p["C"], nu=p["nu"], p=p["p"], eps=p["eps"],
             max_iter=min(p["max_iter"], CAP))
    t.update(more)
    return t


def f64(x):
    return float.fromhex(x)


def same_bits(a, b):
    """Equal bit for bit.  Two NaNs count as equal whatever their sign and
    payload: IEEE 754 leaves both open for the NaN an invalid operation makes
    (r = 0 or inf turns rho / r into 0 / 0 or inf / inf), and the x86 host sets
    the sign bit of that NaN where the GPU clears it."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def assert_same_solution(g, h, what):
    """Two solutions of one task, bit for bit: everything the solve determines
    (the GPU path against the host path; a batch against a task alone)."""
    assert same_bits(g.coef, h.coef), (what, np.flatnonzero(bits(g.coef) != bits(h.coef))[:8])
    assert same_bits(g.rho, h.rho) and same_bits(g.obj, h.obj) and same_bits(g.r, h.r), \
        (what, g.rho, h.rho, g.obj, h.obj, g.r, h.r)
    assert (g.iterations, g.status, g.n_free, g.n_bound) == (h.iterations, h.status, h.n_free, h.n_bound), what


def assert_decisions_close(K, g, h, what):
    """assert_sums_close's bound for the decision values (tests/test_svm_train.py),
    restated for signed coefficients: the GPU adds the l terms coef_a K[s][t_a]
    in a tree, the host in list order, so both are within l 2^-53 sum |term| of
    the exact sum, plus each path's rounding of the final `- rho`."""
    if not len(h.test):
        return
    l = len(h.train)
    assert np.all(np.isfinite(h.coef)), what
    terms = np.abs(K[np.ix_(h.test, h.train)]) @ np.abs(h.coef)
    bound = 2 * l * 2.0 ** -53 * terms + 2.0 ** -53 * (np.abs(g.decision) + np.abs(h.decision))
    err = np.abs(g.decision - h.decision)
    print(f"{what}: decision values worst {err.max():.3g} of bound {bound[err.argmax()]:.3g}")
    assert np.all(np.isfinite(g.decision)) and np.all(err <= bound), what


# tasks sk_svm_solve_batch refuses with SK_ERR_INVALID (svm_check_parameter,
# libsvm/svm.cpp:1499-1615), over the 300-example Gram
def bad_tasks(y):
    pos = [int(k) for k in np.flatnonzero(y > 0)[:3]]
    neg = [int(k) for k in np.flatnonzero(y <= 0)[:3]]
    ten = [int(k) for k in np.flatnonzero(y > 0)[:2]] + [int(k) for k in np.flatnonzero(y <= 0)[:8]]
    bad = {}
    for ty in ("nu_svc", "one_class", "nu_svr"):
        for name, nu in (("nu = 0", 0.0), ("nu < 0", -0.5), ("nu > 1", 1.0 + 2.0 ** -40), ("nu nan", float("nan"))):
            bad[f"{ty}: {name}"] = dict(svm_type=ty, train=[0, 1, 2, 3], nu=nu)
    # 0.5 * 10 / 2 = 2.5 > min(2, 8); at nu = 0.4 it is 2 == 2 and feasible
    bad["nu_svc: nu infeasible"] = dict(svm_type="nu_svc", train=ten, nu=0.5)
    bad["nu_svc: positives only"] = dict(svm_type="nu_svc", train=pos, nu=0.1)
    bad["nu_svc: negatives only"] = dict(svm_type="nu_svc", train=neg, nu=0.1)
    bad["c_svc: positives only"] = dict(svm_type="c_svc", train=pos)
    for ty in ("c_svc", "epsilon_svr", "nu_svr"):
        bad[f"{ty}: C = 0"] = dict(svm_type=ty, train=[0, 1, 2], C=0.0)
        bad[f"{ty}: C < 0"] = dict(svm_type=ty, train=[0, 1, 2], C=-1.0)
    bad["epsilon_svr: p < 0"] = dict(svm_type="epsilon_svr", train=[0, 1, 2], p=-2.0 ** -20)
    for ty in ("c_svc",) + TYPES:
        bad[f"{ty}: eps = 0"] = dict(svm_type=ty, train=[0, 1, 2], eps=0.0)
        bad[f"{ty}: eps < 0"] = dict(svm_type=ty, train=[0, 1, 2], eps=-1e-3)
        bad[f"{ty}: max_iter = 0"] = dict(svm_type=ty, train=[0, 1, 2], max_iter=0)
        bad[f"{ty}: n_train = 1"] = dict(svm_type=ty, train=[0])
        bad[f"{ty}: n_train = 0"] = dict(svm_type=ty, train=[])
        bad[f"{ty}: train index = n"] = dict(svm_type=ty, train=[0, 1, len(y)])
        bad[f"{ty}: train index < 0"] = dict(svm_type=ty, train=[0, 1, -1])
        bad[f"{ty}: test index = n"] = dict(svm_type=ty, train=[0, 1, 2], test=[len(y)])
        bad[f"{ty}: test index < 0"] = dict(svm_type=ty, train=[0, 1, 2], test=[-1])
    return bad


def feasible_edge(y):
    """The twin of "nu_svc: nu infeasible" at nu = 0.4: nu l / 2 == min(n+, n-)."""
    ten = [int(k) for k in np.flatnonzero(y > 0)[:2]] + [int(k) for k in np.flatnonzero(y <= 0)[:8]]
    return dict(svm_type="nu_svc", train=ten, nu=0.4)


def bad_targets(targets):
    """(targets, task): an SVR target that is not finite, inside the training list only."""
    out = {}
    for name, v in (("inf", float("inf")), ("-inf", float("-inf")), ("nan", float("nan"))):
        t = targets.copy()
        t[2] = v
        for ty in SVR:
            out[f"{ty}: target {name}"] = (t, dict(svm_type=ty, train=[0, 1, 2]))
    return out


# ---- the size-class edges, on the max_train integer Gram of tests/test_svm_train.py
EDGE_SEED, EDGE_TARGET_SEED = 0x5A17C001, 0x5A17D0FF
# nu, C, p and eps of the edge batches: the host path converges in at most
# 1,040 iterations at every size (33 / 38 for nu-SVC / one-class), far under 40,000
EDGE_PARAMS = {"nu_svc": dict(nu=0.25), "one_class": dict(nu=0.25), "epsilon_svr": dict(C=2.0 ** -6, p=0.5),
               "nu_svr": dict(C=2.0 ** -6, nu=0.5)}


@functools.lru_cache(maxsize=None)
def edge_gram(max_train):
    K, y = svm_ref.int_gram(EDGE_SEED, max_train, 8, 2)
    r = svm_ref.splitmix64_stream(EDGE_TARGET_SEED, max_train)
    return K, y, np.array([(int(v) % 65 - 32) / 4.0 for v in r])


def edge_lengths(ty, bounds):
    """Training-list lengths at the edges of the size classes, which go by
    positions: l for the classifiers, 2 l for the SVR types."""
    if ty in SVR:
        return [2, 32, 33] + [e // 2 + d for e in bounds[:-1] for d in (-1, 0, 1)] + \
            [bounds[-1] // 2 - 1, bounds[-1] // 2]
    return [2, 3, 63, 64, 65] + [v for e in bounds[:-1] for v in (e - 1, e, e + 1)] + [bounds[-1] - 1, bounds[-1]]


def edge_batch(ty, bounds):
    return [dict(train=np.arange(l), test=[0, 1, l // 2], svm_type=ty, eps=1e-3, max_iter=CAP, **EDGE_PARAMS[ty])
            for l in edge_lengths(ty, bounds)]
