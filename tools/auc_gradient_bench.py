#!/usr/bin/env python3
"""The optimizer's cross-validated AUC gradient (sk_auc_gradient_batch,
csrc/kernels/auc_grad.hip) on one MI355X against the host path on 16 threads.

Workload: the SVM bench's (tools/svm_train_bench.py) -- one 2,048-example
integer Gram, 5 folds (the reference's split) x 10 values of C (2^-6 .. 2^3):
50 problems of 1,638 or 1,639 training examples -- with four synthetic
gradient matrices (integer Grams from other seeds).  The folds are trained
once on the GPU (sk_svm_train_batch; the alphas are the host path's bits),
delta comes from sk_auc_delta of the GPU's decision values, and the same 50
gradient problems go to both paths.  The Gram has rank 16, so few examples
are free (n_free is reported per problem) and the conjugate gradient is
short: this workload measures the sums around it.  --ridge R adds R to the
Gram's diagonal and runs the whole measurement a second time: then hundreds
of examples are free and the products P w dominate.

Timed, each the median of --calls calls after --warmup warm-ups:
  gpu batch   the 50 problems in one call: wall time of the call (upload of
              the 32 MB Gram and 134 MB of gradient matrices, kernels,
              download) and the GPU span of its launches (HIP events,
              Context.last_launch_ms)
  host batch  sk_auc_gradient_batch_host on --threads threads
The two paths' cg, fg and d_u are compared bit for bit.  Writes one JSON
document (--out); no pass/fail threshold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stem_kernel_amd as ska  # noqa: E402
from tests import svm_ref  # noqa: E402


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(b)
    return bool(np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan]))


def measure(ctx, K, G, y, Cs, folds, a):
    ps = [dict(train=tr, test=ts, C=c, eps=1e-3, max_iter=a.max_iter) for c in Cs for tr, ts in folds]
    t0 = time.perf_counter()
    sols = ska.svm_train_batch(K, y, ps, ctx=ctx)
    train_ms = (time.perf_counter() - t0) * 1e3
    gp = [dict(train=p["train"], test=p["test"], C=p["C"], alpha=s.alpha, rho=s.rho,
               delta=ska.auc_delta(s.decision, y[p["test"]])[1]) for p, s in zip(ps, sols)]
    wall, span, launches = [], [], 0
    for it in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        gpu = ska.auc_gradient_batch(K, G, y, gp, ctx=ctx)
        t1 = time.perf_counter()
        if it >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            lm = ctx.last_launch_ms()
            span.append(lm["ms_sum"])
            launches = lm["launches"]
    hwall = []
    for it in range(1 + a.calls):
        t0 = time.perf_counter()
        host = ska.auc_gradient_batch(K, G, y, gp, n_threads=a.threads)
        t1 = time.perf_counter()
        if it >= 1:
            hwall.append((t1 - t0) * 1e3)
    same = all(same_bits([g.cg], [h.cg]) and same_bits(g.fg, h.fg) and same_bits(g.d_u, h.d_u) and
               (g.n_free, g.n_bound, g.cg_iterations, g.finite) == (h.n_free, h.n_bound, h.cg_iterations, h.finite)
               for g, h in zip(gpu, host))
    mspan, mwall, mhost = statistics.median(span), statistics.median(wall), statistics.median(hwall)
    # the problem with the most free examples alone: one workgroup against one host thread
    big = max(range(len(gp)), key=lambda k: gpu[k].n_free)
    solo_gpu, solo_host = [], []
    for it in range(1 + 3):
        ska.auc_gradient_batch(K, G, y, [gp[big]], ctx=ctx)
        t0 = time.perf_counter()
        ska.auc_gradient_batch(K, G, y, [gp[big]], n_threads=1)
        t1 = time.perf_counter()
        if it >= 1:
            solo_gpu.append(ctx.last_launch_ms()["ms_sum"])
            solo_host.append((t1 - t0) * 1e3)
    return dict(
        largest_problem=dict(n_free=gpu[big].n_free, n_bound=gpu[big].n_bound, cg_products=gpu[big].cg_iterations,
                             gpu_kernel_ms=statistics.median(solo_gpu),
                             host_one_thread_ms=statistics.median(solo_host),
                             host_thread_over_workgroup=statistics.median(solo_host) / statistics.median(solo_gpu)),
        problems=len(gp), n_train=sorted({len(p["train"]) for p in gp}), all_converged=all(s.converged for s in sols),
        svm_train_batch_wall_ms=train_ms,
        n_free=[g.n_free for g in gpu], n_bound=[g.n_bound for g in gpu],
        cg_products=[g.cg_iterations for g in gpu], finite=[bool(g.finite) for g in gpu],
        outputs_bit_equal_gpu_host=bool(same), launches_per_call=launches,
        gpu_batch_wall_ms=wall, gpu_batch_span_ms=span, host_batch_wall_ms=hwall,
        median_gpu_batch_wall_ms=mwall, median_gpu_batch_span_ms=mspan, median_host_batch_wall_ms=mhost,
        host_over_gpu_span=mhost / mspan, host_over_gpu_wall=mhost / mwall,
    )


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--max-iter", type=int, default=2_000_000)
    ap.add_argument("--ridge", type=float, default=0.0, help="also measure with this added to the Gram's diagonal")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    K, y = svm_ref.int_gram(0x5A17B001, a.n, 16, 4)
    G = np.stack([svm_ref.int_gram(0x5A17B010 + k, a.n, 16, 4)[0] for k in range(4)])
    Cs = [2.0 ** e for e in range(-6, 4)]
    folds = [svm_ref.split(a.n, a.folds, f) for f in range(a.folds)]
    ctx = ska.Context(0)
    res = dict(device="MI355X (gfx950)", n=a.n, folds=a.folds, Cs=Cs, n_params=len(G), eps=1e-3,
               shape=ska.auc_gradient_shape(), calls=a.calls, warmup=a.warmup, host_threads=a.threads,
               rank16=measure(ctx, K, G, y, Cs, folds, a))
    if a.ridge > 0:
        res["ridge"] = dict(added_to_diagonal=a.ridge, **measure(ctx, K + a.ridge * np.eye(a.n), G, y, Cs, folds, a))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
