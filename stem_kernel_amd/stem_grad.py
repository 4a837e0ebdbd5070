"""Gradients of the DAG stem kernels (SuStemKernel, SiStemKernel, their --log
and + string compositions) with respect to loop_gap, beta, stack and covar,
and the hyperparameter optimizer over them: sk_stem_gradients on a GPU context
(csrc/kernels/stem_grad.hip), sk_stem_gradients_host with ctx=None (its value
is bit for bit the reference's).

The per-pair function is StemKernel<ST,MData>::operator()
(stem_kernel_lite/stem_kernel.cpp:14-95) differentiated in forward mode.  The
reference has no such gradient: stem_kernel/train.cpp is an L-BFGS trainer
over a kernel.inside_outside(x, y, params, grad) that was never written.  The
derivative here is the exact derivative of the DP (include/stem_kernel.h,
sk_stem_gradients).

Gradients with respect to the string parameters of the + string kinds (gap,
alpha, match, mismatch) are out of scope: those kinds' values include the
string term, their gradients are the stem part's."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib

_I32P = C.POINTER(C.c_int32)
_F64P = C.POINTER(C.c_double)

# the gradient row's slots, and the live ones of each family of kinds
SLOTS = ("loop_gap", "beta", "stack", "covar")
_SU_KINDS = (_lib.SU_STEM, _lib.SU_STEM_STR, _lib.LSU_STEM, _lib.LSU_STEM_STR)
_SI_KINDS = (_lib.SI_STEM, _lib.SI_STEM_STR)

# The optimizer's bounds.  They are this project's own choice, not the
# reference's (which has no optimizer of these kernels): loop_gap is a
# per-position decay in (0, 1], and the other three must stay positive for
# the kernel to stay a sum of positive terms.
STEM_BOUNDS = dict(loop_gap=(1e-3, 1.0), beta=(1e-3, None), stack=(1e-3, None), covar=(1e-3, None))
C_BOUNDS = (1e-5, None)


def live_slots(kernel):
    """The names of the parameters a stem kind's gradient is taken over, in
    slot order: (loop_gap, beta) for the Su kinds, (loop_gap, stack, covar)
    for the Si kinds.  Any other kind raises ValueError."""
    k = kernel.params.kind
    if k in _SU_KINDS:
        return ("loop_gap", "beta")
    if k in _SI_KINDS:
        return ("loop_gap", "stack", "covar")
    raise ValueError("the stem gradients need a DAG stem kernel (SuStem, SiStem, LSuStem or their + string kinds)")


def _with_params(kernel, **fields):
    """A copy of the kernel with some parameter fields replaced."""
    k = object.__new__(type(kernel))
    k.__dict__.update(kernel.__dict__)
    p = type(kernel.params)()
    C.memmove(C.byref(p), C.byref(kernel.params), C.sizeof(p))
    for name, v in fields.items():
        setattr(p, name, float(v))
    k.params = p
    return k


def stem_last_kernels(ctx) -> dict:
    """Kernels the context's last stem_gradients call launched
    (sk_last_stem_grad): ``su`` (two tangents) and ``si`` (three)."""
    m = C.c_uint32()
    check(lib().sk_last_stem_grad(ctx.handle, C.byref(m)), ctx.handle)
    return dict(su=bool(m.value & 1), si=bool(m.value & 2))


def stem_gradients(ds, kernel, x, y, ys=None, ctx=None, n_threads: int = 0):
    """Value and gradient of a stem kernel for the ordered pairs (ds[x[k]],
    (ys or ds)[y[k]]): returns (values[n], grads[n, 4] = d/d(loop_gap, beta,
    stack, covar)); the slots the kind does not read are +0.0.  Under the log
    kinds a pair with K_stem = 0 has the value -inf and NaN in the loop_gap
    and beta slots.  ctx=None runs the host path on n_threads threads (0:
    all)."""
    live_slots(kernel)
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
        check(lib().sk_stem_gradients_host(ds.handle, ys.handle, *args, int(n_threads), *out))
    else:
        ctx.upload(ds)
        ctx.upload(ys)
        check(lib().sk_stem_gradients(ctx.handle, ds.handle, ys.handle, *args, *out), ctx.handle)
    return val, grad


def stem_gradient_gram(ds, kernel, normalize: bool = False, ctx=None, n_threads: int = 0):
    """The optimizer's Gram and gradient matrices of a dataset under a stem
    kernel: the cells i <= j, mirrored, or with normalize K / sqrt(K_ii K_jj)
    and its derivative (diagonal 1 in K and 0 in G), through
    shard.assemble_gradients.  Returns (K[n, n], G[4, n, n]) with G in slot
    order.  Raises ValueError on a non-finite value (a log kind over a pair
    with K_stem = 0)."""
    from .shard import assemble_gradients
    n = len(ds)
    iu, ju = np.triu_indices(n)
    val, grad = stem_gradients(ds, kernel, iu, ju, ctx=ctx, n_threads=n_threads)
    if not np.all(np.isfinite(val)):
        k = int(np.flatnonzero(~np.isfinite(val))[0])
        raise ValueError(f"stem_gradient_gram: K({iu[k]}, {ju[k]}) = {val[k]} is not finite")
    return assemble_gradients(iu, ju, val, grad, n, normalize)


def stem_auc_objective(ds, kernel, labels, n_folds: int, C: float, normalize: bool = False, eps: float = 1e-3,
                       max_iter=None, shrinking: bool = False, ctx=None, n_threads: int = 0):
    """One optimizer step for a stem kernel: stem_gradient_gram, then
    svm.auc_objective over it (optimizer/optimizer.cpp:45-77).  Returns
    (f, g, records) with g over (C, the kind's live parameters): the dead
    slots, always zero, are dropped."""
    from . import svm
    live = live_slots(kernel)
    K, G = stem_gradient_gram(ds, kernel, normalize, ctx=ctx, n_threads=n_threads)
    f, g, records = svm.auc_objective(K, G, labels, n_folds, C, eps=eps, ctx=ctx, n_threads=n_threads,
                                      shrinking=shrinking,
                                      max_iter=svm.DEFAULT_MAX_ITER if max_iter is None else max_iter)
    keep = [0] + [1 + SLOTS.index(s) for s in live]
    return f, np.asarray(g)[keep], records


def optimize_stem(ds, labels, kernel=None, C: float = 1.0, n_folds: int = 10, normalize: bool = False, ctx=None,
                  eps: float = 1e-3, max_iter=None, n_threads: int = 0, callback=None, shrinking: bool = False,
                  **options):
    """Minimise minus the cross-validated smoothed AUC of a dataset over
    (C, the kernel's live stem parameters) with svm.optimize, from the
    kernel's parameters (default SuStemKernel()).  The bounds are this
    project's own choice, not the reference's: loop_gap in [1e-3, 1],
    beta >= 1e-3, stack >= 1e-3, covar >= 1e-3 and C >= 1e-5.
    callback(step, x, f, g) is called after every evaluation.  Returns
    (result, the kernel at the optimum); result.x[0] is C.  ctx=None runs
    every step on the host path."""
    from . import svm
    from .kernel_matrix import SuStemKernel
    kernel = SuStemKernel() if kernel is None else kernel
    live = live_slots(kernel)
    step = [0]

    def at(p):
        return _with_params(kernel, **dict(zip(live, p)))

    def objective(x):
        f, g, _ = stem_auc_objective(ds, at(x[1:]), labels, n_folds, float(x[0]), normalize=normalize, eps=eps,
                                     max_iter=max_iter, shrinking=shrinking, ctx=ctx, n_threads=n_threads)
        step[0] += 1
        if callback is not None:
            callback(step[0], np.array(x, dtype=np.float64), f, g)
        return f, g

    x0 = [C] + [getattr(kernel.params, s) for s in live]
    res = svm.optimize(objective, x0, bounds=[C_BOUNDS] + [STEM_BOUNDS[s] for s in live], **options)
    return res, at(res.x[1:])
