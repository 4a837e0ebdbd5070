#!/usr/bin/env python3
"""How far the reference's conjugate gradient moves under a reordering of the
free support vectors, measured with the host path
(sk_auc_gradient_batch_host).

RBF Grams over n random points in the plane (n = 60 and 150, three values of
gamma), four values of C, five folds: 120 folds.  Every fold is trained once;
its gradient problem is then solved twice, with the training list (and alpha
with it) in the given order and reversed.  The two problems are the same
mathematically -- only the order of the free examples, so the rounding of
every sum, differs.  Prints, per class of n_free, how many folds there are
and the median and the largest relative movement of cg and fg, and whether
equal product counts help."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stem_kernel_amd as ska  # noqa: E402
from tests import svm_ref  # noqa: E402


def main():
    rows = []
    for n in (60, 150):
        r = svm_ref.splitmix64_stream(0x5A17E000 + n, 3 * n)
        pts = np.stack([(r[:n] % np.uint64(2001)).astype(float) / 500 - 2,
                        (r[n:2 * n] % np.uint64(2001)).astype(float) / 500 - 2], axis=1)
        noise = (r[2 * n:] % np.uint64(1000)).astype(float) / 1000
        y = np.where((pts ** 2).sum(axis=1) + noise < 2.5, 1.0, -1.0)
        D = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
        for gamma in (0.1, 0.5, 2.0):
            K = np.exp(-gamma * D)
            G = np.stack([-D * K])
            for C in (0.25, 1.0, 8.0, 64.0):
                folds = [ska.cv_split(n, 5, f) for f in range(5)]
                sols = ska.svm_train_batch(K, y, [dict(train=tr, test=ts, C=C) for tr, ts in folds])
                fwd, rev = [], []
                for (tr, ts), s in zip(folds, sols):
                    d = ska.auc_delta(s.decision, y[ts])[1]
                    fwd.append(dict(train=tr, test=ts, C=C, alpha=s.alpha, rho=s.rho, delta=d))
                    rev.append(dict(train=tr[::-1], test=ts, C=C, alpha=s.alpha[::-1], rho=s.rho, delta=d))
                for a, b in zip(ska.auc_gradient_batch(K, G, y, fwd), ska.auc_gradient_batch(K, G, y, rev)):
                    rel = lambda u, v: abs(u - v) / max(abs(u), abs(v), 1e-300)
                    rows.append((a.n_free, rel(a.cg, b.cg), rel(a.fg[0], b.fg[0]),
                                 a.cg_iterations == b.cg_iterations))
    print(f"{len(rows)} folds")
    for name, pick in (("n_free <= 10", lambda r: r[0] <= 10), ("n_free > 10", lambda r: r[0] > 10),
                       ("n_free > 10, equal product counts", lambda r: r[0] > 10 and r[3]),
                       ("n_free > 10, unequal product counts", lambda r: r[0] > 10 and not r[3])):
        sel = [r for r in rows if pick(r)]
        if not sel:
            print(f"{name}: none")
            continue
        for what, k in (("cg", 1), ("fg", 2)):
            v = np.array([r[k] for r in sel])
            print(f"{name:38s} {len(sel):3d} folds  {what}: median {np.median(v):.1e}  max {v.max():.1e}  "
                  f"moved > 1e-6: {(v > 1e-6).sum()}")


if __name__ == "__main__":
    main()
