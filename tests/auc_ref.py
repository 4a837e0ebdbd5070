"""Inputs of the AUC-gradient tests: the matrices of
tests/golden/auc_gradient.json materialised (integer Grams from their seeds,
tests/svm_ref.int_gram; the RBF Gram and its gradient matrix stored), the
fixture's loader, crafted alphas with a wanted number of free and bound
examples, and the problems as auc_gradient_batch takes them."""
import functools
import json
import os

import numpy as np

from tests import svm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "auc_gradient.json")


def materialise(m):
    """(matrix, labels or None) of a fixture matrix record."""
    if m["kind"] == "int":
        K, y = svm_ref.int_gram(m["seed"], m["n"], m["d"], m["shift"], m["indef"], m["dup"])
        if m.get("asym"):
            # an upper triangle of small integers on top: K[r][c] != K[c][r]
            r, c = np.indices(K.shape)
            K = K + np.triu((7 * r + 3 * c) % 5 - 2, 1) / float(1 << m["shift"])
        return np.ascontiguousarray(K), y
    n = m["n"]
    K = np.array([float.fromhex(v) for v in m["values"]]).reshape(n, n)
    y = np.array(m["labels"], dtype=np.float64) if "labels" in m else None
    return K, y


@functools.lru_cache(maxsize=None)
def fixture():
    """(problems, matrices) of the fixture, loaded once: matrices[k] = (M, labels)."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    return fx["problems"], [materialise(m) for m in fx["matrices"]]


def hexes(v):
    return np.array([float.fromhex(x) for x in v], dtype=np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def inputs(p, mats):
    """(K, G or None, labels) of a fixture problem."""
    K, y = mats[p["k"]]
    G = np.stack([mats[g][0] for g in p["g"]]) if p["g"] else None
    return K, G, y


def as_problem(p, delta=None):
    """A fixture record as auc_gradient_batch takes it (the fixture's delta
    unless another is given)."""
    return dict(train=p["train"], test=p["test"], C=p["C"], alpha=hexes(p["alpha"]), rho=float.fromhex(p["rho"]),
                delta=hexes(p["delta"]) if delta is None else delta)


def crafted(seed, train, test, C, n_free, n_bound):
    """(alpha, rho, dec) with exactly n_free free and n_bound bound examples
    at positions drawn from `seed`: free alphas C (k + 1) / (n_free + 2),
    bound ones C, the others 0; rho and the decision values in [-2, 2]."""
    l, m = len(train), len(test)
    assert n_free + n_bound <= l
    r = svm_ref.splitmix64_stream(seed, l + m + 1)
    order = np.argsort(r[:l], kind="stable")
    alpha = np.zeros(l)
    for k, pos in enumerate(order[:n_free]):
        alpha[pos] = C * (k + 1) / (n_free + 2)
    alpha[order[n_free:n_free + n_bound]] = C
    dec = (r[l:l + m] % np.uint64(2001)).astype(np.float64) / 500.0 - 2.0
    rho = float(int(r[l + m] % np.uint64(2001))) / 500.0 - 2.0
    return alpha, rho, dec
