"""The reference's rbf_optimizer, poly_optimizer and sigmoid_optimizer
(optimizer/{rbf,poly,sigmoid}_optimizer.cpp) over the engine:

    python -m stem_kernel_amd.optimizer {rbf,poly,sigmoid} [options] training-data

with the reference's flags and defaults (-g 1, -c 1, -e 0.001, --factr 1e10,
--pgtol 1e-5, -v 10; poly: -d 3 -r 0; sigmoid: -r 0) and its per-step output
(optimizer/optimizer.cpp:43-85).  The iterates are SciPy's L-BFGS-B's, not
lbfgsb.c's (svm.optimize): factr and pgtol map to SciPy's ftol = factr *
machine epsilon and gtol.  --host runs every step on host threads instead of
the GPU.  --shrinking trains every fold with libsvm's shrinking, which the
reference's optimizer hardcodes (optimizer/gradient.cpp:224); the default is
without.
"""
from __future__ import annotations

import argparse
import functools
import sys

import numpy as np

from . import features


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m stem_kernel_amd.optimizer", add_help=False,
                                 description="Hyperparameter optimizer for RBF, polynomial and sigmoid kernels")
    ap.add_argument("kernel", choices=("rbf", "poly", "sigmoid"))
    ap.add_argument("--help", "-h", action="help", help="show this message")
    ap.add_argument("--degree", "-d", type=int, default=3, help="set degree in kernel function (poly)")
    ap.add_argument("--gamma", "-g", type=float, default=1.0, help="set gamma in kernel function")
    ap.add_argument("--coef0", "-r", type=float, default=0.0, help="set coef0 in kernel function (poly, sigmoid)")
    ap.add_argument("--cost", "-c", type=float, default=1.0, help="set the parameter C of C-SVC")
    ap.add_argument("--epsilon", "-e", type=float, default=0.001,
                    help="set tolerance of termination criterion for the SVM training")
    ap.add_argument("--factr", type=float, default=1e10,
                    help="set the factor for machine epsilon used for the convergence tolerance of iterations")
    ap.add_argument("--pgtol", type=float, default=1e-5,
                    help="set the tolerance of the maximum gradient of the object function")
    ap.add_argument("--nfold", "-v", type=int, default=10, help="n-fold cross validation mode")
    ap.add_argument("--host", action="store_true", help="run on host threads instead of the GPU")
    ap.add_argument("--device", type=int, default=0, help="GPU ordinal")
    ap.add_argument("--shrinking", action="store_true",
                    help="train with libsvm's shrinking heuristic, as the reference's optimizer does")
    ap.add_argument("--max-steps", type=int, default=None, help="stop after this many evaluations (SciPy's maxfun)")
    ap.add_argument("data", metavar="training-data")
    return ap


def make_kernel(a):
    if a.kernel == "rbf":
        return features.RBFKernel(a.gamma)
    if a.kernel == "poly":
        return features.PolyKernel(a.degree, a.gamma, a.coef0)
    return features.SigmoidKernel(a.gamma, a.coef0)


def _g(v) -> str:
    return f"{float(v):.6g}"  # an ostream's default formatting of a double


def print_step(step, x, f, g, out=None, n_folds: int = 0) -> None:
    """One step as Optimizer::optimize prints it: it prints -f and -g of the
    values it minimises (f = minus the summed AUC)."""
    out = sys.stdout if out is None else out
    out.write(f"=== Step {step} ===\n- calculate a kernel matrix done.\n- gradient calculation \n")
    out.write(" x=[ " + "".join(_g(v) + " " for v in x) + "]\n  " + "." * n_folds + " done.\n")
    out.write(f" f= {_g(-f)}\n g=[ " + "".join(_g(-v) + " " for v in g) + "]\n\n")
    out.flush()


def main(argv=None) -> int:
    a = parser().parse_args(argv)
    sys.stdout.write(f'loading "{a.data}"')
    sys.stdout.flush()
    fs = features.FeatureSet.read(a.data)
    print(" done.")
    ctx = None
    if not a.host:
        from .kernel_matrix import Context
        ctx = Context(a.device)
    options = dict(ftol=a.factr * np.finfo(np.float64).eps, gtol=a.pgtol, maxcor=5)
    if a.max_steps is not None:
        options["maxfun"] = a.max_steps
    res, best = features.optimize_features(fs, make_kernel(a), C=a.cost, n_folds=a.nfold, ctx=ctx, eps=a.epsilon,
                                           callback=functools.partial(print_step, n_folds=a.nfold),
                                           shrinking=a.shrinking, **options)
    print("\nOptimized Parameters:")
    names = ", ".join(f"{k}={_g(v)}" for k, v in zip(best.names[:1], best.params[:1]))
    tail = "".join(f" {k}={_g(v)}" for k, v in zip(best.names[1:], best.params[1:]))
    print(f"  C={_g(res.x[0])}, {names}{tail}")
    if ctx is not None:
        ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
