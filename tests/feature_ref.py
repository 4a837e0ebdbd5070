"""Shared pieces of the feature-vector Gram tests: the golden fixture
(tests/golden/feature_gram.json and .npz, from the reference's own kernels
through tools/make_golden_feature_gram.py) and deterministic feature sets."""
import json
import os

import numpy as np

import stem_kernel_amd as ska

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FEATURE_FILE = os.path.join(GOLDEN, "features_small.txt")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def full(upper, n):
    """The symmetric matrix of an upper triangle stored row by row."""
    M = np.zeros((n, n))
    iu = np.triu_indices(n)
    M[iu] = upper
    M.T[iu] = M[iu]
    return M


_cache = {}


def golden():
    """labels, vectors, D and per (kernel, setting) a dict with the kernel
    object, K and G -- parsed once."""
    if "g" not in _cache:
        with open(os.path.join(GOLDEN, "feature_gram.json")) as f:
            g = json.load(f)
        n = len(g["labels"])
        mats = np.load(os.path.join(GOLDEN, g["matrices"]))
        cases = []
        for k, c in enumerate(g["kernels"]):
            p = [float.fromhex(v) for v in c["params"]]
            kern = {"rbf": lambda: ska.RBFKernel(*p), "poly": lambda: ska.PolyKernel(c["degree"], *p),
                    "sigmoid": lambda: ska.SigmoidKernel(*p)}[c["kernel"]]()
            cases.append(dict(name=f"{c['kernel']} degree={c['degree']} params={p}", kernel=kern,
                              K=full(mats[f"K{k}"], n), G=np.stack([full(m, n) for m in mats[f"G{k}"]])))
        _cache["g"] = dict(labels=g["labels"], vectors=g["vectors"], D=full(mats["D"], n), cases=cases, n=n)
    return _cache["g"]


def kernels():
    """One of each kernel at two settings (a polynomial degree 1, and an even
    degree with negative gamma d + coef0)."""
    return [ska.RBFKernel(0.25), ska.RBFKernel(0.002), ska.PolyKernel(1, 0.7, 0.3), ska.PolyKernel(4, 0.05, -1.0),
            ska.SigmoidKernel(0.02, 0.1), ska.SigmoidKernel(0.1, -0.5)]


def random_set(n, d, seed, density=1.0, spread=1, empty_rows=(), labels=True):
    """n examples over d columns (indices 1 + k * spread), each entry present
    with the given density, values multiples of 1/512 in [-2, 2]; the rows in
    empty_rows hold nothing.  Every column is used by at least one example
    when density is 1."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-1024, 1025, size=(n, d)) / 512.0
    X[X == 0] = 0.5
    if density < 1.0:
        X[rng.random((n, d)) >= density] = 0.0
    for r in empty_rows:
        X[r] = 0.0
    nz = X != 0
    row_ptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))])
    index = 1 + np.nonzero(nz)[1].astype(np.int64) * spread
    lab = np.where(np.arange(n) % 2 == 0, 1, -1) if labels else None
    return ska.FeatureSet.from_arrays(row_ptr, index, X[nz], lab), X


def rel_close(got, ref, tol=1e-6):
    """The project's parity bound: |got - ref| <= tol |ref|, and where ref is 0,
    |got| <= tol x the matrix's largest magnitude.  Returns the worst ratio to
    the bound (<= 1 passes)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.where(ref != 0, np.abs(ref), np.max(np.abs(ref)) if ref.size else 0.0)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / (tol * scale))
    return float(np.max(ratio)) if ratio.size else 0.0


def ulps(got, ref):
    """The largest distance in units in the last place between two arrays of
    finite doubles of equal sign pattern (0 where the bits are equal)."""
    a = bits(got).astype(np.int64)
    b = bits(ref).astype(np.int64)
    a = np.where(a < 0, np.int64(-2 ** 63) - a, a)
    b = np.where(b < 0, np.int64(-2 ** 63) - b, b)
    return int(np.max(np.abs(a - b))) if a.size else 0
