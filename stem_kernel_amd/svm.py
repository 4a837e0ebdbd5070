"""Two-class C-SVC training on a precomputed Gram (sk_svm_train_batch): what
replaces `svm-train -t 4` on the printed matrix and the per-fold solves of the
reference's optimizer.  Many (training subset, C) problems over one Gram are
solved in one call: on the GPU with a Context (one workgroup per problem), on
host threads without one.  libsvm's SMO solver without shrinking; see
include/stem_kernel.h for the arithmetic contract."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import SvmProblem, SvmSolution, check, lib

# The cap on SMO iterations every problem carries (the reference's loop has
# none); reaching it is reported in the solution's status, not raised.  The
# cap bounds how long one kernel can hold a GPU: a workgroup of the largest
# class takes about 8 us per iteration (measured, l = 1,638), so the default
# ends a problem that does not converge after about 8 s.  Hard problems need
# more -- the reference's solver takes 5.85M iterations for l = 1,638,
# C = 1000, eps = 1e-6 -- and say so with max_iter; 10^7 iterations (the cap
# of libsvm's later releases) would be a kernel of 80 s.
DEFAULT_MAX_ITER = 1_000_000
STATUS = {0: "converged", 1: "not converged", 2: "no working pair"}


def svm_train_shape() -> dict:
    """Size classes of the GPU solver (sk_svm_train_shape): n_train <=
    bounds[c] runs in class c; max_train is the longest list it takes."""
    b = (C.c_int32 * 4)()
    nc, mx = C.c_int32(), C.c_int32()
    check(lib().sk_svm_train_shape(b, C.byref(nc), C.byref(mx)))
    return {"bounds": [int(b[c]) for c in range(nc.value)], "max_train": mx.value}


class SVMSolution:
    """One solved problem: alpha (>= 0, in training order, not multiplied by
    y), rho, obj, iterations, status ("converged", "not converged" when
    max_iter was reached, "no working pair" for a Gram that is not finite),
    n_free, n_bound, the decision values of the problem's test list, and the
    problem's train, test, Cp and Cn."""

    def __init__(self, train, test, labels, alpha, decision, s, Cp=None, Cn=None):
        self.train, self.test, self.labels = train, test, labels
        self.Cp, self.Cn = Cp, Cn
        self.alpha, self.decision = alpha, decision
        self.rho, self.obj = float(s.rho), float(s.obj)
        self.iterations = int(s.iterations)
        self.status = STATUS.get(int(s.status), str(int(s.status)))
        self.converged = int(s.status) == 0
        self.n_free, self.n_bound = int(s.n_free), int(s.n_bound)

    def __repr__(self):
        return (f"SVMSolution(l={len(self.train)}, {self.status}, iterations={self.iterations}, "
                f"rho={self.rho:.6g}, obj={self.obj:.6g}, n_free={self.n_free}, n_bound={self.n_bound})")

    def save(self, path: str) -> None:
        """The model in svm_save_model's text format (sk_svm_model_write);
        SVMModel(path) reads it back."""
        lab = np.ascontiguousarray(self.labels, dtype=np.float64)
        check(lib().sk_svm_model_write(str(path).encode(), lab.ctypes.data_as(_lib._F64P), len(lab),
                                       self.train.ctypes.data_as(_lib._I32P), len(self.train),
                                       self.alpha.ctypes.data_as(_lib._F64P), self.rho))

    def model(self, path: str):
        """save(path), loaded as an SVMModel."""
        from .kernel_matrix import SVMModel
        self.save(path)
        return SVMModel(path)


def _problem(p, default_train):
    if not isinstance(p, dict):
        raise TypeError("a problem is a dict: train, test, C or Cp/Cn, eps, max_iter")
    unknown = set(p) - {"train", "test", "C", "Cp", "Cn", "eps", "max_iter"}
    if unknown:
        raise TypeError(f"unknown problem keys {sorted(unknown)}")
    train = default_train if p.get("train") is None else p["train"]
    train = np.ascontiguousarray(train, dtype=np.int32).reshape(-1)
    test = np.ascontiguousarray([] if p.get("test") is None else p["test"], dtype=np.int32).reshape(-1)
    c = float(p.get("C", 1.0))
    return (train, test, float(p.get("Cp", c)), float(p.get("Cn", c)), float(p.get("eps", 1e-3)),
            int(p.get("max_iter", DEFAULT_MAX_ITER)))


def svm_train_batch(K, labels, problems: Sequence[dict], ctx=None, n_threads: int = 0):
    """Solve every problem of `problems` over the Gram K (n x n) with the
    labels' signs as classes; returns one SVMSolution per problem.  A problem
    is a dict with train (indices into K, default all), test (indices whose
    decision values are wanted), C or Cp and Cn (default 1), eps (default
    1e-3) and max_iter (default DEFAULT_MAX_ITER).  ctx: a Context runs the
    batch on its GPU; None runs it on n_threads host threads (0 = all)."""
    K = np.ascontiguousarray(K, dtype=np.float64)
    if K.ndim != 2 or K.shape[0] != K.shape[1]:
        raise ValueError("K must be a square matrix")
    n = K.shape[0]
    labels = np.ascontiguousarray(labels, dtype=np.float64).reshape(-1)
    if len(labels) != n:
        raise ValueError("one label per row of K")
    every = np.arange(n, dtype=np.int32)
    ps = [_problem(p, every) for p in problems]
    arr = (SvmProblem * max(len(ps), 1))()
    for a, (train, test, cp, cn, eps, mi) in zip(arr, ps):
        a.train, a.n_train = train.ctypes.data_as(_lib._I32P), len(train)
        a.test, a.n_test = (test.ctypes.data_as(_lib._I32P) if len(test) else None), len(test)
        a.Cp, a.Cn, a.eps, a.max_iter = cp, cn, eps, mi
    aoff = np.concatenate([[0], np.cumsum([len(p[0]) for p in ps])]).astype(np.int64)
    doff = np.concatenate([[0], np.cumsum([len(p[1]) for p in ps])]).astype(np.int64)
    alpha = np.zeros(max(int(aoff[-1]), 1))
    dec = np.zeros(max(int(doff[-1]), 1))
    sol = (SvmSolution * max(len(ps), 1))()
    args = (K.ctypes.data_as(_lib._F64P), n, labels.ctypes.data_as(_lib._F64P), arr, len(ps))
    outs = (alpha.ctypes.data_as(_lib._F64P), dec.ctypes.data_as(_lib._F64P), sol)
    if ctx is None:
        check(lib().sk_svm_train_batch_host(*args, int(n_threads), *outs))
    else:
        check(lib().sk_svm_train_batch(ctx.handle, *args, *outs), ctx.handle)
    return [SVMSolution(p[0], p[1], labels, alpha[aoff[k]:aoff[k + 1]].copy(), dec[doff[k]:doff[k + 1]].copy(),
                        sol[k], p[2], p[3]) for k, p in enumerate(ps)]


def svm_train(K, labels, C: float = 1.0, train=None, test=None, eps: float = 1e-3,
              max_iter: int = DEFAULT_MAX_ITER, Cp: Optional[float] = None, Cn: Optional[float] = None,
              ctx=None) -> SVMSolution:
    """One C-SVC problem (svm_train_batch with a single entry)."""
    p = dict(train=train, test=test, Cp=C if Cp is None else Cp, Cn=C if Cn is None else Cn, eps=eps,
             max_iter=max_iter)
    return svm_train_batch(K, labels, [p], ctx=ctx)[0]


def cv_split(n: int, n_folds: int, fold: int):
    """The reference's split (Optimizer::split, optimizer/optimizer.cpp:99-116):
    example j is tested in fold j % n_folds and trained on in the others."""
    idx = np.arange(n, dtype=np.int32)
    return idx[idx % n_folds != fold], idx[idx % n_folds == fold]


def _auc(dec, pos):
    """The exact AUC: pairs (positive, negative) ranked right, ties half."""
    p, q = dec[pos], dec[~pos]
    if len(p) == 0 or len(q) == 0:
        return float("nan")
    d = p[:, None] - q[None, :]
    return float(((d > 0).sum() + 0.5 * (d == 0).sum()) / d.size)


class CrossValidation:
    """cross_validate's result: Cs, folds [(train, test)], solutions[c][f],
    decision[c][f] (the test examples' decision values), and per C the
    accuracy (all test examples pooled; a decision value > 0 predicts label
    > 0), the AUC (mean over the folds that test both classes) and whether
    every fold converged."""

    def __init__(self, Cs, folds, solutions, labels):
        self.Cs, self.folds, self.solutions = list(Cs), folds, solutions
        self.decision = [[s.decision for s in row] for row in solutions]
        self.accuracy, self.auc, self.converged = [], [], []
        for row in solutions:
            hit = tot = 0
            aucs = []
            for s, (_, test) in zip(row, folds):
                pos = labels[test] > 0
                hit += int(((s.decision > 0) == pos).sum())
                tot += len(test)
                aucs.append(_auc(s.decision, pos))
            aucs = [a for a in aucs if a == a]
            self.accuracy.append(hit / tot if tot else float("nan"))
            self.auc.append(float(np.mean(aucs)) if aucs else float("nan"))
            self.converged.append(all(s.converged for s in row))


def cross_validate(K, labels, n_folds: int, Cs, eps: float = 1e-3, max_iter: int = DEFAULT_MAX_ITER,
                   ctx=None, n_threads: int = 0) -> CrossValidation:
    """n_folds-fold cross-validation for every C of Cs in one batch: the
    len(Cs) * n_folds problems of the reference's split.  ctx=None runs the
    host path."""
    labels = np.ascontiguousarray(labels, dtype=np.float64).reshape(-1)
    n = len(labels)
    if not 2 <= n_folds <= n:
        raise ValueError("n_folds must be in [2, n]")
    Cs = [float(c) for c in Cs]
    folds = [cv_split(n, n_folds, f) for f in range(n_folds)]
    ps = [dict(train=tr, test=ts, C=c, eps=eps, max_iter=max_iter) for c in Cs for tr, ts in folds]
    flat = svm_train_batch(K, labels, ps, ctx=ctx, n_threads=n_threads)
    sols = [flat[k * n_folds:(k + 1) * n_folds] for k in range(len(Cs))]
    return CrossValidation(Cs, folds, sols, labels)
