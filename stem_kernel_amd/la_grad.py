"""Gradients of the protein local-alignment kernel (LAKernel) and the
hyperparameter optimizer over them: sk_la_protein_gradients on a GPU context
(csrc/kernels/la_protein_grad.hip), sk_la_protein_gradients_host with
ctx=None (bit for bit the reference's arithmetic).

The per-pair function is the reference's
BPLAKernel<double,AAMData>::compute_gradients (bpla_kernel.cpp:385-401) with
p_left = p_right = 0, p_unpair = 1 and alpha = 1.  Its value is NOT the value
``Context.gram`` / ``Context.pairs`` return for an LAKernel (operator()): the
forward model of compute_gradients weights alignment starts differently
(on one pair of 200-residue sequences 903,381 against 304,108) and is not
symmetric in (x, y).  It is the model the reference's optimizer
differentiates, as ``Context.bpla_gradient_gram``'s K is for RNA, and the K of
``la_gradient_gram`` is this value."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib

_I32P = C.POINTER(C.c_int32)
_F64P = C.POINTER(C.c_double)

# bpla_optimizer.cpp:422-426: beta in [1e-3, 0.3], gap <= 0, ext <= 0
LA_BOUNDS = [(1e-3, 0.3), (None, 0.0), (None, 0.0)]


def _need_exp_kernel(kernel):
    if kernel.params.kind != _lib.AA_LA:
        raise ValueError("the protein LA gradients need LAKernel(SW=False): the SW kernel has no gradient")


def la_grad_shape() -> dict:
    """The longest y (columns) of the GPU gradient call's two paths
    (sk_la_protein_grad_shape): ``code`` for pairs of examples with one
    residue kind per column, ``profile`` for the rest.  x is not limited."""
    a, b = C.c_int32(), C.c_int32()
    check(lib().sk_la_protein_grad_shape(C.byref(a), C.byref(b)))
    return dict(code=a.value, profile=b.value)


def la_gradients(ds, kernel, x, y, ys=None, ctx=None, n_threads: int = 0):
    """compute_gradients for the ordered pairs (ds[x[k]], (ys or ds)[y[k]]):
    returns (values[n], grads[n, 4] = d/d(alpha, beta, gap, ext)); the alpha
    column is +0.0.  values are compute_gradients' return values, not the
    LAKernel's Gram values (see the module docstring), and K(x, y) != K(y, x).
    ctx=None runs the host path on n_threads threads (0: all)."""
    _need_exp_kernel(kernel)
    ys = ds if ys is None else ys
    x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1)
    y = np.ascontiguousarray(y, dtype=np.int32).reshape(-1)
    if x.size != y.size:
        raise ValueError("x and y must have one entry per pair")
    val = np.zeros(x.size, dtype=np.float64)
    grad = np.zeros((x.size, 4), dtype=np.float64)
    args = (C.byref(kernel.params), x.ctypes.data_as(_I32P), y.ctypes.data_as(_I32P), x.size)
    out = (val.ctypes.data_as(_F64P), grad.ctypes.data_as(_F64P))
    if ctx is None:
        check(lib().sk_la_protein_gradients_host(ds.handle, ys.handle, *args, int(n_threads), *out))
    else:
        ctx.upload(ds)
        ctx.upload(ys)
        check(lib().sk_la_protein_gradients(ctx.handle, ds.handle, ys.handle, *args, *out), ctx.handle)
    return val, grad


def la_gradient_gram(ds, kernel, normalize: bool = False, ctx=None, n_threads: int = 0):
    """The optimizer's Gram and gradient matrices of a protein dataset:
    CalcMatrix (bpla_optimizer.cpp:52-126: cells i <= j, mirrored) or, with
    normalize, CalcMatrixN (:128-255; diagonal 1 in K and 0 in G), through
    shard.assemble_gradients.  Returns (K[n, n], G[4, n, n]); G[0] (alpha) is
    zero.  K holds compute_gradients' values, not the LAKernel's Gram."""
    from .shard import assemble_gradients
    n = len(ds)
    iu, ju = np.triu_indices(n)
    val, grad = la_gradients(ds, kernel, iu, ju, ctx=ctx, n_threads=n_threads)
    return assemble_gradients(iu, ju, val, grad, n, normalize)


def la_auc_objective(ds, kernel, labels, n_folds: int, C: float, normalize: bool = False, eps: float = 1e-3,
                     max_iter=None, shrinking: bool = False, ctx=None, n_threads: int = 0):
    """One optimizer step for the protein LA kernel: la_gradient_gram, then
    svm.auc_objective over it (optimizer/optimizer.cpp:45-77).  Returns
    (f, g, records) with g over (C, beta, gap, ext): the alpha entry, always
    zero, is dropped."""
    from . import svm
    K, G = la_gradient_gram(ds, kernel, normalize, ctx=ctx, n_threads=n_threads)
    f, g, records = svm.auc_objective(K, G, labels, n_folds, C, eps=eps, ctx=ctx, n_threads=n_threads,
                                      shrinking=shrinking,
                                      max_iter=svm.DEFAULT_MAX_ITER if max_iter is None else max_iter)
    return f, np.delete(g, 1), records


def optimize_la(ds, labels, kernel=None, C: float = 1.0, n_folds: int = 10, normalize: bool = False, ctx=None,
                eps: float = 1e-3, max_iter=None, n_threads: int = 0, callback=None, shrinking: bool = False,
                **options):
    """Minimise minus the cross-validated smoothed AUC of a protein dataset
    over (C, beta, gap, ext) with svm.optimize, from the kernel's parameters
    (default LAKernel()), under the reference's bounds for them
    (bpla_optimizer.cpp:422-426): beta in [1e-3, 0.3], gap <= 0, ext <= 0
    (and C >= 1e-5).  callback(step, x, f, g) is called after every
    evaluation.  Returns (result, LAKernel at the optimum); result.x[0] is C.
    The iterates are SciPy's L-BFGS-B's, not lbfgsb.c's (see svm.optimize).
    ctx=None runs every step on the host path."""
    from . import svm
    from .kernel_matrix import LAKernel
    kernel = LAKernel() if kernel is None else kernel
    _need_exp_kernel(kernel)
    table = np.array(kernel.params.aa_score_table[:])
    step = [0]

    def at(p):
        return LAKernel(beta=float(p[0]), gap=float(p[1]), ext=float(p[2]), score_table=table, cli_float=False)

    def objective(x):
        f, g, _ = la_auc_objective(ds, at(x[1:]), labels, n_folds, float(x[0]), normalize=normalize, eps=eps,
                                   max_iter=max_iter, shrinking=shrinking, ctx=ctx, n_threads=n_threads)
        step[0] += 1
        if callback is not None:
            callback(step[0], np.array(x, dtype=np.float64), f, g)
        return f, g

    p = kernel.params
    res = svm.optimize(objective, [C, p.beta, p.gap, p.ext], bounds=[(1e-5, None)] + LA_BOUNDS, **options)
    return res, at(res.x[1:])
