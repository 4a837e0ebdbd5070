"""Inputs of the C-SVC training tests: the integer Grams of
tests/golden/svm_train.json regenerated from their seeds (the twin of int_gram
in tests/cpp/svm_train_ref_harness.cpp), the fixture's loader, the
reference's cross-validation split, and what the CPU and the GPU test modules
share: the problems as svm_train_batch takes them, the invalid problems, and
the rounding bounds of rho, obj and the decision values."""
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "svm_train.json")
_GAMMA = np.uint64(0x9E3779B97F4A7C15)


def splitmix64_stream(seed, count):
    """The first `count` outputs of splitmix64 from state `seed` (the state is
    a counter, so the stream is computed at once)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + _GAMMA * np.arange(1, count + 1, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def int_gram(seed, n, d, shift=0, indef=0, dup=0):
    """(K, labels): K = A S A^T / 2^shift with A n x d of integers in [-3, 3],
    S the identity or (indef) alternating signs; labels +1 / -1, the first two
    +1, -1; dup: example 1 is example 0 again.  Every entry is a small multiple
    of 2^-shift: exact in double and in float, with many equal values."""
    r = splitmix64_stream(seed, n * d + n)
    A = (r[: n * d] % np.uint64(7)).astype(np.int64).reshape(n, d) - 3
    if dup:
        A[1] = A[0]
    y = np.where(r[n * d:] & np.uint64(1), 1.0, -1.0)
    y[0], y[1] = 1.0, -1.0
    S = np.where(np.arange(d) % 2 == 1, -1, 1) if indef else np.ones(d, dtype=np.int64)
    K = ((A * S) @ A.T).astype(np.float64) / float(1 << shift)
    return np.ascontiguousarray(K), y


def split(n, ncv, cv):
    """Optimizer::split (optimizer/optimizer.cpp:99-116): (train, test)."""
    idx = np.arange(n)
    return idx[idx % ncv != cv].astype(np.int32), idx[idx % ncv == cv].astype(np.int32)


def load_fixture():
    """The fixture with its Grams materialised: grams[g] = (K, labels)."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    grams = []
    for g in fx["grams"]:
        if g["kind"] == "int":
            K, y = int_gram(g["seed"], g["n"], g["d"], g["shift"], g["indef"], g["dup"])
            assert [int(v) for v in y] == g["labels"]
        else:
            n = g["n"]
            K = np.array([float.fromhex(v) for v in g["values"]]).reshape(n, n)
            y = np.array(g["labels"], dtype=np.float64)
        grams.append((K, y))
    return fx, grams


@functools.lru_cache(maxsize=None)
def fixture():
    """(problems, grams) of the fixture, loaded once."""
    fx, grams = load_fixture()
    return fx["problems"], grams


def hexes(v):
    return np.array([float.fromhex(x) for x in v])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def as_problem(p):
    """A fixture record as svm_train_batch takes it."""
    return dict(train=p["train"], Cp=p["Cp"], Cn=p["Cn"], eps=p["eps"], max_iter=p["max_iter"])


# problems sk_svm_train_batch refuses (SK_ERR_INVALID), over the 300-example Gram
BAD = {
    "train index = n": dict(train=[0, 1, 300]),
    "train index < 0": dict(train=[0, 1, -1]),
    "test index = n": dict(train=[0, 1, 2], test=[300]),
    "test index < 0": dict(train=[0, 1, 2], test=[-1]),
    "eps = 0": dict(train=[0, 1, 2], eps=0.0),
    "eps < 0": dict(train=[0, 1, 2], eps=-1e-3),
    "Cp = 0": dict(train=[0, 1, 2], Cp=0.0, Cn=1.0),
    "Cn < 0": dict(train=[0, 1, 2], Cp=1.0, Cn=-1.0),
    "max_iter = 0": dict(train=[0, 1, 2], max_iter=0),
    "n_train = 1": dict(train=[0]),
    "n_train = 0": dict(train=[]),
}


def one_class_lists(y):
    pos = [int(k) for k in np.flatnonzero(y > 0)[:3]]
    neg = [int(k) for k in np.flatnonzero(y < 0)[:3]]
    return {"positives only": dict(train=pos), "negatives only": dict(train=neg)}


def sum_bounds(K, y, train, Cp, Cn, alpha, unit):
    """unit * sum |term| for rho and for obj, from the terms of those sums
    alone: rho is the mean of y G over the free variables (terms |G_k| /
    n_free, k free), else the midpoint of two y G values (terms |G_k| / 2 of
    the largest); obj is sum alpha (G - 1) / 2.  G = Q^T alpha - 1 with Q's
    float entries (G[k] = sum_a Q_a[k] alpha_a - 1: row t_a of the Gram).
    unit is l 2^-52 against recorded values, 2 l 2^-53 between two paths."""
    t = np.asarray(train)
    ys = np.where(y[t] > 0, 1.0, -1.0)
    Q = (np.outer(ys, ys) * K[np.ix_(t, t)]).astype(np.float32).astype(np.float64)
    G = Q.T @ alpha - 1.0
    C = np.where(ys > 0, Cp, Cn)
    free = (alpha > 0) & (alpha < C)
    rho_b = unit * (np.abs(G[free]).sum() / free.sum() if free.any() else np.abs(G).max())
    obj_b = unit * np.abs(alpha * (G - 1.0)).sum() / 2
    return rho_b, obj_b
