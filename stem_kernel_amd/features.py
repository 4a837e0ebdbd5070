"""Feature-vector Grams: the RBF, polynomial and sigmoid kernels of the
reference's rbf_optimizer, poly_optimizer and sigmoid_optimizer over libsvm
feature files (optimizer/rbf_kernel.cpp, poly_kernel.cpp, sigmoid_kernel.cpp),
with their derivative matrices, on the GPU (csrc/kernels/feature_gram.hip) or
on host threads (csrc/host/feature_gram.cpp).  The dot matrix and the whole
polynomial kernel are the reference's bit for bit on both paths; exp, tanh and
cosh are libm's on the host path and the device library's on the GPU."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import StemKernelError, lib

RBF, POLY, SIGMOID = range(3)


def _check(rc, ctx=None):
    if rc != _lib.SK_OK:
        m = lib().sk_last_error(ctx.handle) if ctx is not None else lib().sk_features_last_error()
        raise StemKernelError(rc, m.decode() if m else "")


def feature_gram_shape() -> dict:
    """The dot kernel's tile edge and k-slice, and the limits of both paths
    (sk_feature_gram_shape): max_n examples per set, max_dense entries of
    examples x used columns per call."""
    t, s, n, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    _check(lib().sk_feature_gram_shape(C.byref(t), C.byref(s), C.byref(n), C.byref(d)))
    return {"tile": t.value, "k_slice": s.value, "max_n": n.value, "max_dense": d.value}


class FeatureSet:
    """Labelled sparse feature vectors (sk_features): what the reference's
    read_data makes of a libsvm feature file."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def _make(cls, call, *args):
        h = C.c_void_p()
        _check(call(*args, C.byref(h)))
        return cls(h)

    @classmethod
    def read(cls, path) -> "FeatureSet":
        return cls._make(lib().sk_features_read, os.fsencode(path))

    @classmethod
    def parse(cls, text) -> "FeatureSet":
        data = text.encode() if isinstance(text, str) else bytes(text)
        return cls._make(lib().sk_features_parse, data, len(data))

    @classmethod
    def from_arrays(cls, row_ptr, index, value, labels=None) -> "FeatureSet":
        """From CSR arrays: example i holds index[row_ptr[i]:row_ptr[i+1]]
        (>= 0, strictly ascending) with their finite values."""
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64).reshape(-1)
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
        value = np.ascontiguousarray(value, dtype=np.float64).reshape(-1)
        if len(row_ptr) < 1 or len(index) != len(value) or row_ptr[-1] != len(index):
            raise ValueError("row_ptr has n + 1 entries and ends at len(index) == len(value)")
        n = len(row_ptr) - 1
        lab = None
        if labels is not None:
            lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
            if len(lab) != n:
                raise ValueError("one label per example")
        return cls._make(lib().sk_features_create, n, row_ptr.ctypes.data_as(_lib._I64P),
                         index.ctypes.data_as(_lib._I32P), value.ctypes.data_as(_lib._F64P),
                         lab.ctypes.data_as(_lib._I32P) if lab is not None else None)

    @classmethod
    def from_dense(cls, X, labels=None) -> "FeatureSet":
        """From a dense matrix: the nonzero entries of row i, libsvm indices from 1."""
        X = np.asarray(X, dtype=np.float64)
        nz = X != 0
        row_ptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))])
        return cls.from_arrays(row_ptr, np.nonzero(nz)[1] + 1, X[nz], labels)

    @property
    def handle(self):
        return self._h

    @property
    def shape(self):
        """(n examples, used columns, stored entries)"""
        n, d, z = C.c_int32(), C.c_int32(), C.c_int64()
        _check(lib().sk_features_shape(self._h, C.byref(n), C.byref(d), C.byref(z)))
        return n.value, d.value, z.value

    def __len__(self):
        return self.shape[0]

    @property
    def labels(self) -> np.ndarray:
        out = np.zeros(max(len(self), 1), dtype=np.int32)
        _check(lib().sk_features_labels(self._h, out.ctypes.data_as(_lib._I32P)))
        return out[:len(self)]

    def rows(self):
        """(row_ptr, index, value): the examples as CSR arrays."""
        n, _, z = self.shape
        rp, ix, v = np.zeros(n + 1, dtype=np.int64), np.zeros(max(z, 1), dtype=np.int32), np.zeros(max(z, 1))
        _check(lib().sk_features_rows(self._h, rp.ctypes.data_as(_lib._I64P), ix.ctypes.data_as(_lib._I32P),
                                      v.ctypes.data_as(_lib._F64P)))
        return rp, ix[:z], v[:z]

    def close(self):
        if self._h:
            lib().sk_features_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _FeatureKernel:
    kind = -1
    degree = 0
    names = ()

    @property
    def params(self) -> np.ndarray:
        return np.array([getattr(self, k) for k in self.names], dtype=np.float64)

    def with_params(self, p):
        """The same kernel with other continuous parameters."""
        new = type(self).__new__(type(self))
        new.__dict__.update(self.__dict__)
        for k, v in zip(self.names, p):
            setattr(new, k, float(v))
        return new

    # the reference CLIs' bounds: gamma >= 1e-5, coef0 unbounded
    @property
    def bounds(self):
        return [(1e-5, None) if k == "gamma" else (None, None) for k in self.names]

    def __repr__(self):
        args = ([f"degree={self.degree}"] if self.kind == POLY else []) + [f"{k}={getattr(self, k)!r}" for k in self.names]
        return f"{type(self).__name__}({', '.join(args)})"


class RBFKernel(_FeatureKernel):
    """exp(-gamma |x - y|^2) (rbf_optimizer: -g 1)."""
    kind, names = RBF, ("gamma",)

    def __init__(self, gamma: float = 1.0):
        self.gamma = float(gamma)


class PolyKernel(_FeatureKernel):
    """(gamma x.y + coef0)^degree (poly_optimizer: -d 3 -g 1 -r 0)."""
    kind, names = POLY, ("gamma", "coef0")

    def __init__(self, degree: int = 3, gamma: float = 1.0, coef0: float = 0.0):
        if int(degree) != degree or degree < 0:
            raise ValueError("degree is an integer >= 0")
        self.degree, self.gamma, self.coef0 = int(degree), float(gamma), float(coef0)


class SigmoidKernel(_FeatureKernel):
    """tanh(gamma x.y + coef0) (sigmoid_optimizer: -g 1 -r 0)."""
    kind, names = SIGMOID, ("gamma", "coef0")

    def __init__(self, gamma: float = 1.0, coef0: float = 0.0):
        self.gamma, self.coef0 = float(gamma), float(coef0)


def _f64(a):
    return a.ctypes.data_as(_lib._F64P)


def feature_dots(fs: FeatureSet, ys: FeatureSet = None, ctx=None, n_threads: int = 0) -> np.ndarray:
    """The dot matrix D[i][j] = dot(fs_i, ys_j) (ys None: fs with itself):
    libsvm's sparse merge, bit for bit, on either path.  With a Context the
    matrix is computed once and stays resident on its device."""
    out = np.zeros((len(fs), len(fs if ys is None else ys)))
    yh = None if ys is None else ys.handle
    if ctx is None:
        _check(lib().sk_feature_dots_host(fs.handle, yh, int(n_threads), _f64(out)))
    else:
        _check(lib().sk_feature_dots(ctx.handle, fs.handle, yh, _f64(out)), ctx)
    return out


def feature_gram(fs: FeatureSet, kernel: _FeatureKernel, ctx=None, n_threads: int = 0):
    """(K, G): the Gram of the set and its derivative matrices with respect to
    the kernel's parameters, G[P][n][n] (CM::calculate_matrix).  ctx: a Context
    runs it on its GPU; None on n_threads host threads (0 = all)."""
    n = len(fs)
    p = kernel.params
    K, G = np.zeros((n, n)), np.zeros((len(p), n, n))
    if ctx is None:
        _check(lib().sk_feature_gram_host(fs.handle, kernel.kind, kernel.degree, _f64(p), int(n_threads), _f64(K),
                                          _f64(G)))
    else:
        _check(lib().sk_feature_gram(ctx.handle, fs.handle, kernel.kind, kernel.degree, _f64(p), _f64(K), _f64(G)),
               ctx)
    return K, G


def feature_gram_cross(test: FeatureSet, train: FeatureSet, kernel: _FeatureKernel, ctx=None,
                       n_threads: int = 0) -> np.ndarray:
    """The rectangular K(test, train), for predicting with a trained model."""
    p = kernel.params
    K = np.zeros((len(test), len(train)))
    if ctx is None:
        _check(lib().sk_feature_gram_cross_host(test.handle, train.handle, kernel.kind, kernel.degree, _f64(p),
                                                int(n_threads), _f64(K)))
    else:
        _check(lib().sk_feature_gram_cross(ctx.handle, test.handle, train.handle, kernel.kind, kernel.degree, _f64(p),
                                           _f64(K)), ctx)
    return K


def feature_auc_objective(fs: FeatureSet, kernel: _FeatureKernel, n_folds: int, C: float, eps: float = 1e-3,
                          max_iter=None, ctx=None, n_threads: int = 0, shrinking: bool = False):
    """One step of Optimizer::optimize (optimizer/optimizer.cpp:45-77) for a
    feature-vector kernel: feature_gram, then svm.auc_objective over it.
    Returns (f, g, records) with g over (C, the kernel's parameters).
    shrinking=True trains as the reference's optimizer does."""
    from . import svm
    K, G = feature_gram(fs, kernel, ctx=ctx, n_threads=n_threads)
    return svm.auc_objective(K, G, fs.labels, n_folds, C, eps=eps, ctx=ctx, n_threads=n_threads,
                             max_iter=svm.DEFAULT_MAX_ITER if max_iter is None else max_iter, shrinking=shrinking)


def optimize_features(fs: FeatureSet, kernel: _FeatureKernel, C: float = 1.0, n_folds: int = 10, ctx=None,
                      eps: float = 1e-3, max_iter=None, n_threads: int = 0, callback=None, shrinking: bool = False,
                      **options):
    """The reference's rbf / poly / sigmoid optimizer: minimise minus the
    cross-validated smoothed AUC over (C, the kernel's parameters) with
    svm.optimize, under the reference's bounds (C and gamma >= 1e-5, coef0
    unbounded).  callback(step, x, f, g) is called after every evaluation.
    Returns (result, kernel at the optimum); result.x[0] is C.  The iterates
    are SciPy's L-BFGS-B's, not lbfgsb.c's (see svm.optimize).  shrinking=True
    trains every fold with libsvm's shrinking, as the reference does."""
    from . import svm
    step = [0]

    def objective(x):
        f, g, _ = feature_auc_objective(fs, kernel.with_params(x[1:]), n_folds, float(x[0]), eps=eps,
                                        max_iter=max_iter, ctx=ctx, n_threads=n_threads, shrinking=shrinking)
        step[0] += 1
        if callback is not None:
            callback(step[0], np.array(x, dtype=np.float64), f, g)
        return f, g

    res = svm.optimize(objective, np.concatenate([[C], kernel.params]), bounds=[(1e-5, None)] + kernel.bounds,
                       **options)
    return res, kernel.with_params(res.x[1:])
