"""What the C-SVC shrinking tests share: the fixture
tests/golden/svm_train_shrink.json (the reference's own solver run with
shrinking = 1, made by tools/make_golden_svm_shrink.py) with its Grams
materialised, and the comparison of a solution with a fixture record."""
import functools
import json
import os

import numpy as np

from tests import svm_ref
from tests.svm_ref import bits, hexes

FIXTURE = os.path.join(svm_ref.ROOT, "tests", "golden", "svm_train_shrink.json")
INFO = ("shrink_calls", "shrunk_calls", "min_active", "unshrunk", "regrown", "reconstructions", "resumed")


@functools.lru_cache(maxsize=None)
def fixture():
    """(problems, grams) of the fixture, loaded once; grams[g] = (K, labels)."""
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
        grams.append((K, y))
    return fx["problems"], grams


def assert_is_the_record(s, p):
    """Solution s is fixture record p bit for bit: alphas, rho, obj,
    iterations, status and every counter."""
    alpha = hexes(p["alpha"])
    assert np.array_equal(bits(s.alpha), bits(alpha)), (p["name"], np.flatnonzero(bits(s.alpha) != bits(alpha))[:8])
    assert s.rho == float.fromhex(p["rho"]) and s.obj == float.fromhex(p["obj"]), p["name"]
    assert s.iterations == p["iterations"], p["name"]
    assert s.status == ("not converged" if p["status"] else "converged"), p["name"]
    assert s.shrink == p["info"], (p["name"], s.shrink, p["info"])
    assert tuple(s.shrink) == INFO


def assert_same(a, b, what):
    """Two solutions of one problem: everything the solve determines, info included."""
    assert np.array_equal(bits(a.alpha), bits(b.alpha)), (what, np.flatnonzero(bits(a.alpha) != bits(b.alpha))[:8])
    assert (a.rho, a.obj, a.iterations, a.status, a.n_free, a.n_bound) == \
        (b.rho, b.obj, b.iterations, b.status, b.n_free, b.n_bound), what
    assert a.shrink == b.shrink, (what, a.shrink, b.shrink)
