#!/usr/bin/env python3
"""Batched C-SVC training (sk_svm_train_batch, csrc/kernels/svm_smo.hip) on
one MI355X against the host path on 16 threads.

Workload: model selection over one 2,048-example Gram -- 5 folds (the
reference's split) x 10 values of C (2^-6 .. 2^3), eps 1e-3: 50 problems of
1,638 or 1,639 training examples, each with its fold's test list.  The Gram
is an integer Gram (tests/svm_ref.py: rank 16, random labels, so every
problem is hard for its C and the iteration counts spread over two orders of
magnitude).

Timed, each the median of --calls calls after --warmup warm-ups:
  gpu batch      the 50 problems in one call: wall time of the call (upload
                 of the 32 MB Gram, kernels, download) and the GPU span of its
                 kernel launches (HIP events, Context.last_launch_ms)
  host batch     sk_svm_train_batch_host on --threads threads, same problems
and once: every problem in a call of its own on the GPU (kernel time of one
workgroup alone: iterations/s per workgroup, and what the batch gains over
running them one after another).  Iterations/s per card is the batch's total
iterations over its GPU span.  The alphas of the two paths are compared bit
for bit.  Writes one JSON document (--out).  For scale, the reference
Solver's single-core time on one of these problems is what
tools/make_golden_svm_train.py prints (DESIGN.md records it).

--shrinking measures the same 50 problems with libsvm's shrinking on
(sk_svm_train_batch_ex) instead: GPU span and wall time of the batch, the
iterations, what the shrinking did (sk_svm_shrink_info; per problem the
smallest active size, and its minimum and mean over the batch), the host
path's time, and GPU against host bit for bit; and once in the same process
the batch with shrinking off.  --commit-runs and --parent-runs name JSON
documents written by this tool without --shrinking on the same day, by this
commit and by its parent commit: their median spans are recorded, with the
parent's run-to-run spread (largest minus smallest), and whether shrinking
off has become slower than the parent by more than that spread.  With --out
the record goes under the key "shrinking" of that document, whose other keys
are kept.

--svm-type nu_svc | one_class | epsilon_svr | nu_svr measures the same 50-task
batch as that formulation (sk_svm_solve_batch, without shrinking): the five
folds times a grid of ten values -- the nu grid (--nu, default 0.05 .. 0.5,
which has to be feasible for every fold's labels) for nu_svc and one_class,
the C grid for the SVR types (p = 0.1; nu = the first --nu value for nu_svr).
The SVR targets are multiples of 1/4 in [-8, 8] from a splitmix64 stream.
Recorded: GPU span and wall time of the batch, the host path's wall time on
--threads threads, the iterations, and GPU against host bit for bit.  With
--out the record goes under the key <svm_type> of that document, whose other
keys are kept.

--default-record measures nothing: it merges JSON documents this tool wrote
without options (the default C-SVC bench) on one machine, --parent-runs by the
parent commit and --commit-runs by this one, into the key
"c_svc_default_bench" of --out: every run's median GPU span, the parent's
lowest and highest, and whether this commit's runs lie within them."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--max-iter", type=int, default=2_000_000)
    ap.add_argument("--out", default="")
    ap.add_argument("--shrinking", action="store_true", help="measure the batch with shrinking on (see above)")
    ap.add_argument("--commit-runs", nargs="*", default=[], help="JSON of runs without --shrinking, this commit")
    ap.add_argument("--parent-runs", nargs="*", default=[], help="JSON of runs without --shrinking, parent commit")
    ap.add_argument("--svm-type", default="", choices=["", "nu_svc", "one_class", "epsilon_svr", "nu_svr"],
                    help="measure the batch as this formulation (see above)")
    ap.add_argument("--nu", type=float, nargs="*", default=[0.05 * k for k in range(1, 11)],
                    help="the nu grid of nu_svc and one_class; its first value is nu_svr's nu")
    ap.add_argument("--default-record", action="store_true",
                    help="merge --parent-runs and --commit-runs into --out (see above); no GPU")
    a = ap.parse_args()
    if a.default_record:
        return default_record(a)
    K, y = svm_ref.int_gram(0x5A17B001, a.n, 16, 4)
    Cs = [2.0 ** e for e in range(-6, 4)]
    folds = [svm_ref.split(a.n, a.folds, f) for f in range(a.folds)]
    if a.svm_type:
        return formulation_record(a, ska.Context(0), K, y, Cs, folds)
    ps = [dict(train=tr, test=ts, C=c, eps=1e-3, max_iter=a.max_iter) for c in Cs for tr, ts in folds]
    ctx = ska.Context(0)
    if a.shrinking:
        return shrinking_record(a, ctx, K, y, ps)

    wall, span = [], []
    for it in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        gpu = ska.svm_train_batch(K, y, ps, ctx=ctx)
        t1 = time.perf_counter()
        if it >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            span.append(ctx.last_launch_ms()["ms_sum"])
    hwall = []
    for it in range(1 + a.calls):
        t0 = time.perf_counter()
        host = ska.svm_train_batch(K, y, ps, n_threads=a.threads)
        t1 = time.perf_counter()
        if it >= 1:
            hwall.append((t1 - t0) * 1e3)
    same = all(np.array_equal(g.alpha.view(np.int64), h.alpha.view(np.int64)) and g.iterations == h.iterations
               for g, h in zip(gpu, host))
    iters = [s.iterations for s in gpu]
    solo_ms = []
    for p in ps:  # one workgroup alone on the card
        ska.svm_train_batch(K, y, [p], ctx=ctx)
        solo_ms.append(ctx.last_launch_ms()["ms_sum"])
    rate = [i / (ms * 1e-3) for i, ms in zip(iters, solo_ms)]
    mspan, mwall, mhost = statistics.median(span), statistics.median(wall), statistics.median(hwall)
    res = dict(
        device="MI355X (gfx950)", n=a.n, folds=a.folds, Cs=Cs, problems=len(ps), eps=1e-3,
        n_train=sorted({len(p["train"]) for p in ps}), shape=ska.svm_train_shape(),
        calls=a.calls, warmup=a.warmup, host_threads=a.threads,
        iterations=iters, total_iterations=int(sum(iters)), all_converged=all(s.converged for s in gpu),
        alphas_bit_equal_gpu_host=bool(same),
        gpu_batch_wall_ms=wall, gpu_batch_span_ms=span, host_batch_wall_ms=hwall,
        median_gpu_batch_wall_ms=mwall, median_gpu_batch_span_ms=mspan, median_host_batch_wall_ms=mhost,
        host_over_gpu_span=mhost / mspan, host_over_gpu_wall=mhost / mwall,
        solo_kernel_ms=solo_ms, solo_kernel_ms_sum=float(sum(solo_ms)),
        batch_gain_over_one_after_another=float(sum(solo_ms)) / mspan,
        iterations_per_s_per_workgroup=dict(min=min(rate), median=statistics.median(rate), max=max(rate)),
        us_per_iteration_one_workgroup=1e6 / statistics.median(rate),
        iterations_per_s_per_card=sum(iters) / (mspan * 1e-3),
        row_cache="not built: no LDS cache of Q rows in this kernel, so no hit rate",
        accuracy=ska.CrossValidation(Cs, folds, [gpu[k * a.folds:(k + 1) * a.folds] for k in range(len(Cs))],
                                     y).accuracy,
    )
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def timed_batch(a, ctx, K, y, ps, **kw):
    """(solutions, wall ms, span ms) of --calls calls after --warmup warm-ups."""
    wall, span = [], []
    for it in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        sols = ska.svm_train_batch(K, y, ps, ctx=ctx, **kw)
        t1 = time.perf_counter()
        if it >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            span.append(ctx.last_launch_ms()["ms_sum"])
    return sols, wall, span


def formulation_record(a, ctx, K, y, Cs, folds):
    ty = a.svm_type
    if ty in ("nu_svc", "one_class"):
        grid, key = list(a.nu), "nu"
        if ty == "nu_svc":
            for tr, _ in folds:
                n_pos = int((y[tr] > 0).sum())
                assert max(grid) * len(tr) / 2 <= min(n_pos, len(tr) - n_pos), "a nu of the grid is infeasible"
        ps = [dict(train=tr, test=ts, svm_type=ty, nu=v, eps=1e-3, max_iter=a.max_iter) for v in grid for tr, ts in folds]
        targets = y
    else:
        grid, key = Cs, "C"
        r = svm_ref.splitmix64_stream(0x5A17B002, a.n)
        targets = np.array([(int(v) % 65 - 32) / 4.0 for v in r])
        ps = [dict(train=tr, test=ts, svm_type=ty, C=c, p=0.1, nu=a.nu[0], eps=1e-3, max_iter=a.max_iter)
              for c in Cs for tr, ts in folds]
    gpu, wall, span = timed_batch(a, ctx, K, targets, ps)
    launches = ctx.last_launch_ms()["launches"]
    hwall = []
    for it in range(1 + a.calls):
        t0 = time.perf_counter()
        host = ska.svm_train_batch(K, targets, ps, n_threads=a.threads)
        t1 = time.perf_counter()
        if it >= 1:
            hwall.append((t1 - t0) * 1e3)
    same = all(np.array_equal(g.coef.view(np.int64), h.coef.view(np.int64)) and g.iterations == h.iterations and
               (g.rho, g.obj, g.r, g.n_free, g.n_bound) == (h.rho, h.obj, h.r, h.n_free, h.n_bound)
               for g, h in zip(gpu, host))
    iters = [s.iterations for s in gpu]
    mspan, mwall, mhost = statistics.median(span), statistics.median(wall), statistics.median(hwall)
    rec = dict(
        device="MI355X (gfx950)", svm_type=ty, grid={key: grid}, n=a.n, folds=a.folds, tasks=len(ps), eps=1e-3,
        n_train=sorted({len(p["train"]) for p in ps}), positions_per_example=2 if ty.endswith("svr") else 1,
        calls=a.calls, warmup=a.warmup, host_threads=a.threads, launches=launches,
        iterations=iters, total_iterations=int(sum(iters)), all_converged=all(s.converged for s in gpu),
        bit_equal_gpu_host=bool(same),
        gpu_batch_wall_ms=wall, gpu_batch_span_ms=span, host_batch_wall_ms=hwall,
        median_gpu_batch_wall_ms=mwall, median_gpu_batch_span_ms=mspan, median_host_batch_wall_ms=mhost,
        host_over_gpu_span=mhost / mspan, host_over_gpu_wall=mhost / mwall,
        us_per_iteration_longest_task=mspan * 1e3 / max(max(iters), 1),
    )
    doc = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc[ty] = rec
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


def default_record(a):
    if not (a.out and a.parent_runs and a.commit_runs):
        sys.exit("--default-record needs --out, --parent-runs and --commit-runs")

    def load(paths):
        docs = []
        for path in paths:
            with open(path) as f:
                docs.append(json.load(f))
        return docs

    parent, mine = load(a.parent_runs), load(a.commit_runs)
    ps, cs = [d["median_gpu_batch_span_ms"] for d in parent], [d["median_gpu_batch_span_ms"] for d in mine]
    rec = dict(
        what="median GPU span of the default (C-SVC) bench, tools/svm_train_bench.py without options, one entry per run",
        parent_commit_span_ms=ps, this_commit_span_ms=cs, parent_low_ms=min(ps), parent_high_ms=max(ps),
        parent_spread_ms=max(ps) - min(ps), this_commit_within_parent_runs=bool(min(ps) <= min(cs) and max(cs) <= max(ps)),
        this_commit_minus_parent_mean_ms=statistics.mean(cs) - statistics.mean(ps),
        total_iterations=dict(parent=[d["total_iterations"] for d in parent],
                              this_commit=[d["total_iterations"] for d in mine]),
        alphas_bit_equal_gpu_host=dict(parent=[d["alphas_bit_equal_gpu_host"] for d in parent],
                                       this_commit=[d["alphas_bit_equal_gpu_host"] for d in mine]),
        gpu_batch_span_ms=dict(parent=[d["gpu_batch_span_ms"] for d in parent],
                               this_commit=[d["gpu_batch_span_ms"] for d in mine]))
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc["c_svc_default_bench"] = rec
    print(json.dumps(rec, indent=1))
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


def shrinking_record(a, ctx, K, y, ps):
    off, off_wall, off_span = timed_batch(a, ctx, K, y, ps)
    on, wall, span = timed_batch(a, ctx, K, y, ps, shrinking=True)
    hwall = []
    for it in range(1 + a.calls):
        t0 = time.perf_counter()
        host = ska.svm_train_batch(K, y, ps, n_threads=a.threads, shrinking=True)
        t1 = time.perf_counter()
        if it >= 1:
            hwall.append((t1 - t0) * 1e3)
    same = all(np.array_equal(g.alpha.view(np.int64), h.alpha.view(np.int64)) and g.iterations == h.iterations and
               (g.rho, g.obj) == (h.rho, h.obj) and g.shrink == h.shrink for g, h in zip(on, host))
    iters, iters_off = [s.iterations for s in on], [s.iterations for s in off]
    min_active = [s.shrink["min_active"] for s in on]
    rec = dict(
        problems=len(ps), calls=a.calls, warmup=a.warmup, host_threads=a.threads,
        iterations=iters, total_iterations=int(sum(iters)), total_iterations_shrinking_off=int(sum(iters_off)),
        all_converged=all(s.converged for s in on), bit_equal_gpu_host=bool(same),
        gpu_batch_wall_ms=wall, gpu_batch_span_ms=span, host_batch_wall_ms=hwall,
        median_gpu_batch_wall_ms=statistics.median(wall), median_gpu_batch_span_ms=statistics.median(span),
        median_host_batch_wall_ms=statistics.median(hwall),
        us_per_iteration_longest_problem=statistics.median(span) * 1e3 / max(iters),
        same_process_shrinking_off=dict(gpu_batch_span_ms=off_span, median_gpu_batch_span_ms=statistics.median(off_span),
                                        us_per_iteration_longest_problem=statistics.median(off_span) * 1e3 / max(iters_off)),
        min_active_per_problem=min_active, min_active_min=min(min_active), min_active_mean=float(np.mean(min_active)),
        n_train=sorted({len(p["train"]) for p in ps}),
        shrink_calls=[s.shrink["shrink_calls"] for s in on], shrunk_calls=[s.shrink["shrunk_calls"] for s in on],
        unshrunk=int(sum(s.shrink["unshrunk"] for s in on)), regrown=int(sum(s.shrink["regrown"] for s in on)),
        reconstructions=int(sum(s.shrink["reconstructions"] for s in on)),
        resumed=int(sum(s.shrink["resumed"] for s in on)),
        alphas_differ_from_shrinking_off=int(sum(not np.array_equal(g.alpha, o.alpha) for g, o in zip(on, off))),
    )

    def spans(paths):
        out = []
        for path in paths:
            with open(path) as f:
                out.append(json.load(f)["median_gpu_batch_span_ms"])
        return out

    if a.commit_runs and a.parent_runs:
        mine, parent = spans(a.commit_runs), spans(a.parent_runs)
        spread = max(parent) - min(parent)
        rec["shrinking_off_same_day"] = dict(
            what="median GPU span of the batch without shrinking, one entry per run of this tool",
            this_commit_span_ms=mine, parent_commit_span_ms=parent, parent_spread_ms=spread,
            this_commit_median_ms=statistics.median(mine), parent_median_ms=statistics.median(parent),
            slower_than_parent_by_more_than_the_spread=bool(statistics.median(mine) - statistics.median(parent) > spread))
    doc = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc["shrinking"] = rec
    text = json.dumps(doc if a.out else rec, indent=1)
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
