"""Two-class C-SVC training on a precomputed Gram (sk_svm_train_batch): what
replaces `svm-train -t 4` on the printed matrix and the per-fold solves of the
reference's optimizer.  Many (training subset, C) problems over one Gram are
solved in one call: on the GPU with a Context (one workgroup per problem), on
host threads without one.  libsvm's SMO solver, without shrinking by default
and with it on request (shrinking=True: what `svm-train` and the reference's
optimizer run); see include/stem_kernel.h for the arithmetic contract."""
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
# sk_svm_type, libsvm's numbering
SVM_TYPES = {"c_svc": 0, "nu_svc": 1, "one_class": 2, "epsilon_svr": 3, "nu_svr": 4}


def svm_train_shape() -> dict:
    """Size classes of the GPU solver (sk_svm_train_shape): n_train <=
    bounds[c] runs in class c; max_train is the longest list it takes."""
    b = (C.c_int32 * 4)()
    nc, mx = C.c_int32(), C.c_int32()
    check(lib().sk_svm_train_shape(b, C.byref(nc), C.byref(mx)))
    return {"bounds": [int(b[c]) for c in range(nc.value)], "max_train": mx.value}


def svm_solve_shape() -> dict:
    """The longest training list the GPU solver takes per svm_type
    (sk_svm_solve_shape): svm_train_shape's max_train, and half of it for the
    SVR types, whose 2 l positions go by svm_train_shape's bounds."""
    m = (C.c_int32 * 5)()
    check(lib().sk_svm_solve_shape(m))
    return {name: int(m[t]) for name, t in SVM_TYPES.items()}


class SVMSolution:
    """One solved problem: alpha (>= 0, in training order, not multiplied by
    y), rho, obj, iterations, status ("converged", "not converged" when
    max_iter was reached, "no working pair" for a Gram that is not finite),
    n_free, n_bound, the decision values of the problem's test list, the
    problem's train, test, Cp and Cn, and shrink: sk_svm_shrink_info as a dict
    (shrink_calls, shrunk_calls, min_active, unshrunk, regrown,
    reconstructions, resumed; without shrinking min_active = l, zeros else).

    A problem solved with an svm_type (sk_svm_solve_batch) has svm_type, coef
    (what goes into a model's sv_coef: alpha y, alpha y / r, alpha, or alpha -
    alpha* by type), r (Solver_NU's, 0 for the plain solver), C, nu and p;
    rho and obj are what svm_train_one leaves; n_free and n_bound count the
    solver's positions (2 l for the SVR types); labels holds the targets;
    alpha is None unless the type is c_svc (coef * y) or one_class (coef).
    Without an svm_type: svm_type "c_svc", coef = alpha y, r = 0."""

    def __init__(self, train, test, labels, alpha, decision, s, Cp=None, Cn=None, shrink=None, svm_type="c_svc",
                 coef=None, nu=None, p=None):
        self.train, self.test, self.labels = train, test, labels
        self.Cp, self.Cn = Cp, Cn
        self.svm_type, self.nu, self.p = svm_type, nu, p
        self.r = float(getattr(s, "r", 0.0))
        if coef is None:
            coef = alpha * np.where(np.asarray(labels)[train] > 0, 1.0, -1.0)
        self.coef = coef
        self.alpha, self.decision = alpha, decision
        self.rho, self.obj = float(s.rho), float(s.obj)
        self.iterations = int(s.iterations)
        self.status = STATUS.get(int(s.status), str(int(s.status)))
        self.converged = int(s.status) == 0
        self.n_free, self.n_bound = int(s.n_free), int(s.n_bound)
        self.shrink = None if shrink is None else {k: int(getattr(shrink, k)) for k, _ in shrink._fields_}

    def __repr__(self):
        return (f"SVMSolution(l={len(self.train)}, {self.status}, iterations={self.iterations}, "
                f"rho={self.rho:.6g}, obj={self.obj:.6g}, n_free={self.n_free}, n_bound={self.n_bound})")

    def save(self, path: str) -> None:
        """The model in svm_save_model's text format, of the solution's
        svm_type (sk_svm_model_write, sk_svm_model_write_ex); SVMModel(path)
        reads it back."""
        lab = np.ascontiguousarray(self.labels, dtype=np.float64)
        ty = SVM_TYPES[getattr(self, "svm_type", "c_svc")]
        if ty == 0 and self.alpha is not None:
            check(lib().sk_svm_model_write(str(path).encode(), lab.ctypes.data_as(_lib._F64P), len(lab),
                                           self.train.ctypes.data_as(_lib._I32P), len(self.train),
                                           self.alpha.ctypes.data_as(_lib._F64P), self.rho))
            return
        coef = np.ascontiguousarray(self.coef, dtype=np.float64)
        check(lib().sk_svm_model_write_ex(str(path).encode(), ty, lab.ctypes.data_as(_lib._F64P), len(lab),
                                          self.train.ctypes.data_as(_lib._I32P), len(self.train),
                                          coef.ctypes.data_as(_lib._F64P), self.rho))

    def model(self, path: str):
        """save(path), loaded as an SVMModel."""
        from .kernel_matrix import SVMModel
        self.save(path)
        return SVMModel(path)


def _problem(p, default_train):
    if not isinstance(p, dict):
        raise TypeError("a problem is a dict: train, test, C or Cp/Cn, eps, max_iter, svm_type, nu, p")
    unknown = set(p) - {"train", "test", "C", "Cp", "Cn", "eps", "max_iter", "svm_type", "nu", "p"}
    if unknown:
        raise TypeError(f"unknown problem keys {sorted(unknown)}")
    train = default_train if p.get("train") is None else p["train"]
    train = np.ascontiguousarray(train, dtype=np.int32).reshape(-1)
    test = np.ascontiguousarray([] if p.get("test") is None else p["test"], dtype=np.int32).reshape(-1)
    c = float(p.get("C", 1.0))
    return (train, test, float(p.get("Cp", c)), float(p.get("Cn", c)), float(p.get("eps", 1e-3)),
            int(p.get("max_iter", DEFAULT_MAX_ITER)))


def _marshal(K, n, labels, ps, struct, fill, solution):
    """The parsed problems ps (train and test first in each) as a call sees
    them: (the leading arguments with the array of `struct`, whose other
    fields fill(a, p) sets; the offsets of each problem's slice of the two
    outputs; the outputs; the array of `solution` records)."""
    arr = (struct * max(len(ps), 1))()
    for a, p in zip(arr, ps):
        train, test = p[0], p[1]
        a.train, a.n_train = train.ctypes.data_as(_lib._I32P), len(train)
        a.test, a.n_test = (test.ctypes.data_as(_lib._I32P) if len(test) else None), len(test)
        fill(a, p)
    aoff = np.concatenate([[0], np.cumsum([len(p[0]) for p in ps])]).astype(np.int64)
    doff = np.concatenate([[0], np.cumsum([len(p[1]) for p in ps])]).astype(np.int64)
    out = np.zeros(max(int(aoff[-1]), 1))
    dec = np.zeros(max(int(doff[-1]), 1))
    args = (K.ctypes.data_as(_lib._F64P), n, labels.ctypes.data_as(_lib._F64P), arr, len(ps))
    return args, aoff, doff, out, dec, (solution * max(len(ps), 1))()


def _solve_tasks(K, n, labels, problems, every, ctx, n_threads):
    """The problems that name an svm_type: sk_svm_solve_batch[_host]."""
    ps = []
    for p in problems:
        train, test, _, _, eps, mi = _problem(p, every)
        if ("Cp" in p or "Cn" in p) and p["svm_type"] != "c_svc":
            raise ValueError("Cp and Cn belong to c_svc; the other types take C")
        if p["svm_type"] == "c_svc" and p.get("Cp", p.get("C", 1.0)) != p.get("Cn", p.get("C", 1.0)):
            raise ValueError("a c_svc problem with svm_type takes one C; leave svm_type out for Cp != Cn")
        c = float(p.get("C", p.get("Cp", 1.0)))
        ps.append((train, test, SVM_TYPES[p["svm_type"]], c, float(p.get("nu", 0.5)), float(p.get("p", 0.1)), eps,
                   mi, p["svm_type"]))
    def fill(a, p):
        a.svm_type, a.C, a.nu, a.p, a.eps, a.max_iter = p[2:8]

    args, aoff, doff, coef, dec, sol = _marshal(K, n, labels, ps, _lib.SvmTask, fill, _lib.SvmTaskSolution)
    outs = (coef.ctypes.data_as(_lib._F64P), dec.ctypes.data_as(_lib._F64P), sol)
    if ctx is None:
        check(lib().sk_svm_solve_batch_host(*args, int(n_threads), *outs))
    else:
        check(lib().sk_svm_solve_batch(ctx.handle, *args, *outs), ctx.handle)
    res = []
    for k, (train, test, ty, c, nu, tube, _, _, name) in enumerate(ps):
        cf = coef[aoff[k]:aoff[k + 1]].copy()
        alpha = cf * np.where(labels[train] > 0, 1.0, -1.0) if ty == 0 else cf if ty == 2 else None
        res.append(SVMSolution(train, test, labels, alpha, dec[doff[k]:doff[k + 1]].copy(), sol[k], c, c,
                               svm_type=name, coef=cf, nu=nu, p=tube))
    return res


def svm_train_batch(K, labels, problems: Sequence[dict], ctx=None, n_threads: int = 0, shrinking: bool = False):
    """Solve every problem of `problems` over the Gram K (n x n) with the
    labels' signs as classes; returns one SVMSolution per problem.  A problem
    is a dict with train (indices into K, default all), test (indices whose
    decision values are wanted), C or Cp and Cn (default 1), eps (default
    1e-3) and max_iter (default DEFAULT_MAX_ITER).  ctx: a Context runs the
    batch on its GPU; None runs it on n_threads host threads (0 = all).
    shrinking: run libsvm's solver with its shrinking heuristic (the whole
    call; the reference's Solve(..., shrinking = 1) bit for bit) instead of
    without (shrinking = 0, the default).

    A problem may name an svm_type ("c_svc", "nu_svc", "one_class",
    "epsilon_svr", "nu_svr": svm_train_one, libsvm/svm.cpp:245-300) with nu
    (default 0.5) and p (default 0.1, epsilon_svr's tube); then every problem
    of the call has to name one, `labels` holds class labels for the
    classifiers and real targets for the SVR types, and the batch goes through
    sk_svm_solve_batch.  Those types are solved without shrinking only:
    shrinking=True with a type other than c_svc is refused.  Problems without
    svm_type go through sk_svm_train_batch as before."""
    K = np.ascontiguousarray(K, dtype=np.float64)
    if K.ndim != 2 or K.shape[0] != K.shape[1]:
        raise ValueError("K must be a square matrix")
    n = K.shape[0]
    labels = np.ascontiguousarray(labels, dtype=np.float64).reshape(-1)
    if len(labels) != n:
        raise ValueError("one label per row of K")
    every = np.arange(n, dtype=np.int32)
    typed = [isinstance(p, dict) and p.get("svm_type") is not None for p in problems]
    if any(typed):
        if not all(typed):
            raise ValueError("either every problem of a call names an svm_type or none does")
        for p in problems:
            if p["svm_type"] not in SVM_TYPES:
                raise ValueError(f"svm_type {p['svm_type']!r}: one of {sorted(SVM_TYPES)}")
        others = sorted({p["svm_type"] for p in problems} - {"c_svc"})
        if shrinking and others:
            raise ValueError(f"shrinking=True is built for c_svc only, not for {', '.join(others)}: "
                             "solve those with shrinking=False")
        if not shrinking:
            return _solve_tasks(K, n, labels, problems, every, ctx, n_threads)
        problems = [{k: v for k, v in p.items() if k not in ("svm_type", "nu", "p")} for p in problems]
    ps = [_problem(p, every) for p in problems]
    def fill(a, p):
        a.Cp, a.Cn, a.eps, a.max_iter = p[2:6]

    args, aoff, doff, alpha, dec, sol = _marshal(K, n, labels, ps, SvmProblem, fill, SvmSolution)
    info =(_lib.SvmShrinkInfo * max(len(ps), 1))()
    outs = (alpha.ctypes.data_as(_lib._F64P), dec.ctypes.data_as(_lib._F64P), sol, info)
    flag = 1 if shrinking else 0
    if ctx is None:
        check(lib().sk_svm_train_batch_host_ex(*args, int(n_threads), flag, *outs))
    else:
        check(lib().sk_svm_train_batch_ex(ctx.handle, *args, flag, *outs), ctx.handle)
    return [SVMSolution(p[0], p[1], labels, alpha[aoff[k]:aoff[k + 1]].copy(), dec[doff[k]:doff[k + 1]].copy(),
                        sol[k], p[2], p[3], info[k]) for k, p in enumerate(ps)]


def svm_train(K, labels, C: float = 1.0, train=None, test=None, eps: float = 1e-3,
              max_iter: int = DEFAULT_MAX_ITER, Cp: Optional[float] = None, Cn: Optional[float] = None,
              ctx=None, shrinking: bool = False, svm_type: Optional[str] = None, nu: float = 0.5,
              p: float = 0.1) -> SVMSolution:
    """One problem (svm_train_batch with a single entry): C-SVC, or with
    svm_type one of the five formulations with nu and p."""
    if svm_type is not None:
        q = dict(train=train, test=test, C=C, eps=eps, max_iter=max_iter, svm_type=svm_type, nu=nu, p=p)
        if Cp is not None:
            q["Cp"] = Cp
        if Cn is not None:
            q["Cn"] = Cn
        return svm_train_batch(K, labels, [q], ctx=ctx, shrinking=shrinking)[0]
    p = dict(train=train, test=test, Cp=C if Cp is None else Cp, Cn=C if Cn is None else Cn, eps=eps,
             max_iter=max_iter)
    return svm_train_batch(K, labels, [p], ctx=ctx, shrinking=shrinking)[0]


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
                   ctx=None, n_threads: int = 0, shrinking: bool = False) -> CrossValidation:
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
    flat = svm_train_batch(K, labels, ps, ctx=ctx, n_threads=n_threads, shrinking=shrinking)
    sols = [flat[k * n_folds:(k + 1) * n_folds] for k in range(len(Cs))]
    return CrossValidation(Cs, folds, sols, labels)


# ---------------------------------------------------------------- the optimizer's AUC gradient
def auc_gradient_shape() -> dict:
    """The GPU path's shape (sk_auc_gradient_shape): n_free <= lds_free keeps
    the KKT matrix in LDS, more keeps it in a device scratch; max_free is the
    most one problem may have; scratch_budget bytes are shared per launch."""
    a, b, s = C.c_int32(), C.c_int32(), C.c_int64()
    check(lib().sk_auc_gradient_shape(C.byref(a), C.byref(b), C.byref(s)))
    return {"lds_free": a.value, "max_free": b.value, "scratch_budget": s.value}


def auc_delta(dec, labels_of_test):
    """(f, delta): the smoothed AUC of the decision values over the test
    list's (positive, negative) pairs and its gradient with respect to them
    (sk_auc_delta; compute_delta, optimizer/gradient.cpp:159-206).  A label
    >= 0 counts as positive here.  One class only: f = 0, delta = 0."""
    dec = np.ascontiguousarray(dec, dtype=np.float64).reshape(-1)
    lab = np.ascontiguousarray(labels_of_test, dtype=np.float64).reshape(-1)
    if len(dec) != len(lab):
        raise ValueError("one label per decision value")
    delta = np.zeros(max(len(dec), 1))
    f = C.c_double()
    check(lib().sk_auc_delta(dec.ctypes.data_as(_lib._F64P), lab.ctypes.data_as(_lib._F64P), len(dec),
                             delta.ctypes.data_as(_lib._F64P), C.byref(f)))
    return f.value, delta[:len(dec)]


class AUCGradient:
    """One problem's result: cg (d AUC / d C), fg[n_params] (d AUC / d kernel
    parameter), d_u (the solution of solve_d's system, n_free + 1 entries;
    empty when n_free is 0), n_free, n_bound, cg_iterations (products the
    conjugate gradient formed) and finite (False when an output is inf/NaN)."""

    def __init__(self, cg, fg, d_u, info):
        self.cg, self.fg, self.d_u = float(cg), fg, d_u
        self.n_free, self.n_bound = int(info.n_free), int(info.n_bound)
        self.cg_iterations, self.finite = int(info.cg_iterations), bool(info.finite)

    def __repr__(self):
        return (f"AUCGradient(cg={self.cg:.6g}, fg={self.fg}, n_free={self.n_free}, n_bound={self.n_bound}, "
                f"cg_iterations={self.cg_iterations}, finite={self.finite})")


def _auc_problem(p):
    if not isinstance(p, dict):
        raise TypeError("a problem is a dict: train, test, C, alpha, rho, delta")
    unknown = set(p) - {"train", "test", "C", "alpha", "rho", "delta"}
    if unknown:
        raise TypeError(f"unknown problem keys {sorted(unknown)}")
    return (np.ascontiguousarray(p["train"], dtype=np.int32).reshape(-1),
            np.ascontiguousarray(p["test"], dtype=np.int32).reshape(-1), float(p["C"]),
            np.ascontiguousarray(p["alpha"], dtype=np.float64).reshape(-1), float(p["rho"]),
            np.ascontiguousarray(p["delta"], dtype=np.float64).reshape(-1))


def auc_gradient_batch(K, G, labels, problems: Sequence[dict], ctx=None, n_threads: int = 0):
    """The gradient of the smoothed AUC of every problem's held-out examples
    with respect to C and to each kernel parameter (sk_auc_gradient_batch;
    steps 4 and 5 of GradientComputation::compute,
    optimizer/gradient.cpp:107-156).  K is the Gram (n x n), G its derivative
    matrices (n_params x n x n, or None), labels the n labels (none may be
    0).  A problem is a dict with train, test (indices into K), C, alpha (the
    trained fold's, in training order), rho and delta (auc_delta's, in test
    order).  Returns one AUCGradient per problem.  ctx: a Context runs the
    batch on its GPU; None runs it on n_threads host threads (0 = all).  Both
    paths give the same bits."""
    K = np.ascontiguousarray(K, dtype=np.float64)
    if K.ndim != 2 or K.shape[0] != K.shape[1]:
        raise ValueError("K must be a square matrix")
    n = K.shape[0]
    if G is None:
        G = np.zeros((0, n, n))
    G = np.ascontiguousarray(G, dtype=np.float64)
    if G.ndim != 3 or G.shape[1:] != (n, n):
        raise ValueError("G must be n_params matrices of K's shape")
    n_params = G.shape[0]
    labels = np.ascontiguousarray(labels, dtype=np.float64).reshape(-1)
    if len(labels) != n:
        raise ValueError("one label per row of K")
    ps = [_auc_problem(p) for p in problems]
    arr = (_lib.AucProblem * max(len(ps), 1))()
    for a, (train, test, c, alpha, rho, delta) in zip(arr, ps):
        if len(alpha) != len(train) or len(delta) != len(test):
            raise ValueError("one alpha per training example and one delta per test example")
        a.train, a.n_train = train.ctypes.data_as(_lib._I32P), len(train)
        a.test, a.n_test = test.ctypes.data_as(_lib._I32P), len(test)
        a.C, a.rho = c, rho
        a.alpha, a.delta = alpha.ctypes.data_as(_lib._F64P), delta.ctypes.data_as(_lib._F64P)
    doff = np.concatenate([[0], np.cumsum([len(p[0]) + 1 for p in ps])]).astype(np.int64)
    cg = np.zeros(max(len(ps), 1))
    fg = np.zeros((max(len(ps), 1), n_params))
    du = np.zeros(max(int(doff[-1]), 1))
    info = (_lib.AucInfo * max(len(ps), 1))()
    head = (K.ctypes.data_as(_lib._F64P), G.ctypes.data_as(_lib._F64P) if n_params else None, n_params, n,
            labels.ctypes.data_as(_lib._F64P), arr, len(ps))
    outs = (cg.ctypes.data_as(_lib._F64P), fg.ctypes.data_as(_lib._F64P) if n_params else None,
            du.ctypes.data_as(_lib._F64P), info)
    if ctx is None:
        check(lib().sk_auc_gradient_batch_host(*head, int(n_threads), *outs))
    else:
        check(lib().sk_auc_gradient_batch(ctx.handle, *head, *outs), ctx.handle)
    res = []
    for k in range(len(ps)):
        nd = info[k].n_free + 1 if info[k].n_free > 0 else 0
        res.append(AUCGradient(cg[k], fg[k].copy(), du[doff[k]:doff[k] + nd].copy(), info[k]))
    return res


def auc_objective(K, G, labels, n_folds: int, C: float, eps: float = 1e-3, max_iter: int = DEFAULT_MAX_ITER,
                  ctx=None, n_threads: int = 0, shrinking: bool = False):
    """One optimizer step's objective and gradient (Optimizer::optimize,
    optimizer/optimizer.cpp:60-77): over the n_folds folds of cv_split, train
    with C (svm_train_batch with each fold's test list), form auc_delta of
    the held-out decision values and auc_gradient_batch, and sum f -= f0,
    g[0] -= cg, g[1 + p] -= fg[p] in fold order.  Returns (f, g, records):
    minus the summed smoothed AUC, its gradient with respect to (C,
    parameters), and per fold a dict with f, delta, the SVMSolution and the
    AUCGradient.  Training is without shrinking unless shrinking=True, which
    is how the reference's optimizer trains (optimizer/gradient.cpp:224)."""
    labels = np.ascontiguousarray(labels, dtype=np.float64).reshape(-1)
    n = len(labels)
    if not 2 <= n_folds <= n:
        raise ValueError("n_folds must be in [2, n]")
    folds = [cv_split(n, n_folds, f) for f in range(n_folds)]
    sols = svm_train_batch(K, labels, [dict(train=tr, test=ts, C=C, eps=eps, max_iter=max_iter)
                                       for tr, ts in folds], ctx=ctx, n_threads=n_threads, shrinking=shrinking)
    fd = [auc_delta(s.decision, labels[ts]) for s, (_, ts) in zip(sols, folds)]
    grads = auc_gradient_batch(K, G, labels, [dict(train=tr, test=ts, C=C, alpha=s.alpha, rho=s.rho, delta=d)
                                              for (tr, ts), s, (_, d) in zip(folds, sols, fd)],
                               ctx=ctx, n_threads=n_threads)
    n_params = 0 if G is None else len(G)
    f, g = 0.0, np.zeros(1 + n_params)
    records = []
    for (f0, d), s, r in zip(fd, sols, grads):
        f -= f0
        g[0] -= r.cg
        for p in range(n_params):
            g[1 + p] -= r.fg[p]
        records.append(dict(f=f0, delta=d, solution=s, gradient=r))
    return f, g, records


def optimize(objective, x0, bounds=None, **options):
    """Minimise objective(x) -> (f, g) over x = (C, kernel parameters...) with
    scipy.optimize.minimize(method="L-BFGS-B") and return its result.  bounds:
    one (low, high) pair per entry of x (None = unbounded); C's lower bound is
    raised to 1e-5, the one the reference sets (optimizer/optimizer.cpp:29).
    This stands in for the reference's f2c lbfgsb.c, which is neither restated
    nor pinned: the iterates are SciPy's, not the reference's.  SciPy is
    imported here, so the package does not depend on it."""
    from scipy.optimize import minimize
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1)
    bounds = [(None, None)] * len(x0) if bounds is None else [tuple(b) for b in bounds]
    if len(bounds) != len(x0):
        raise ValueError("one (low, high) pair per entry of x0")
    lo, hi = bounds[0]
    bounds[0] = (1e-5 if lo is None else max(1e-5, lo), hi)

    def fun(x):
        f, g = objective(x)[:2]
        return float(f), np.asarray(g, dtype=np.float64)

    return minimize(fun, x0, jac=True, method="L-BFGS-B", bounds=bounds, options=options or None)
