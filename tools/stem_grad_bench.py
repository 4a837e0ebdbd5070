#!/usr/bin/env python3
"""Throughput of the stem gradient kernel (sk_stem_gradients,
csrc/kernels/stem_grad.hip) on one MI355X, beside the forward Gram of the same
set and the host path.

  set       the bench's synthetic single sequences (splitmix64 ACGU, L = 200,
            seed of bench.py's NS configuration), kind SK_SU_STEM
  gradient  the upper triangle of --n (1,024) examples in one call; if a
            first run over 256 examples projects more than --budget-s (60)
            seconds for it, the 256-example figures stand and the document
            says so
  forward   sk_gram over the same set in the same process (existing code:
            dag_stem.hip's register classes), the floor
  host      sk_stem_gradients_host on --host-threads (16) threads over the
            first --host-pairs (2,048) pairs of the same list, wall clock

Each GPU figure is the median of --calls calls after --warmup warm-ups, from
the call's GPU span (Context.last_timing).  Writes one JSON document (--out).
--bench-parent / --bench-commit take the JSON result lines of `python bench.py`
on the parent commit and on this one and record them in the same document."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stem_kernel_amd as ska  # noqa: E402
from stem_kernel_amd import provenance  # noqa: E402

NS_SEED = 0x5EED0000 + 2


def gpu_spans(ctx, call, calls, warmup):
    for _ in range(warmup):
        call()
    out = []
    for _ in range(calls):
        call()
        out.append(ctx.last_timing()["stem_ms"])
    return out


def measure(ctx, n, length, a, host):
    seqs = ska.random_sequences(n, length, NS_SEED)
    ds = ska.Dataset.synthetic(seqs, th=0.01, threads=a.host_threads)
    kern = ska.SuStemKernel()
    iu, ju = np.triu_indices(n)
    t0 = time.perf_counter()
    grad_ms = gpu_spans(ctx, lambda: ctx.stem_gradients(ds, kern, iu, ju), a.calls, a.warmup)
    wall = (time.perf_counter() - t0) / (a.calls + a.warmup)
    fwd_ms = gpu_spans(ctx, lambda: ctx.gram(ds, kern), a.calls, a.warmup)
    gm, fm = statistics.median(grad_ms), statistics.median(fwd_ms)
    doc = dict(examples=n, length=length, pairs=int(iu.size), kernels=ska.stem_grad.stem_last_kernels(ctx),
               gpu_ms=grad_ms, median_ms=gm, pairs_per_s=iu.size / (gm * 1e-3), wall_s_per_call=wall,
               forward_gram=dict(gpu_ms=fwd_ms, median_ms=fm, pairs_per_s=iu.size / (fm * 1e-3)),
               gradient_over_forward=gm / fm)
    if host:
        hp = min(a.host_pairs, iu.size)
        t0 = time.perf_counter()
        ska.stem_gradients(ds, kern, iu[:hp], ju[:hp], n_threads=a.host_threads)
        host_s = time.perf_counter() - t0
        doc["host"] = dict(threads=a.host_threads, pairs=int(hp), subset="the first pairs of the same list",
                           seconds=host_s, pairs_per_s=hp / host_s)
        doc["gpu_over_host_pairs_per_s"] = doc["pairs_per_s"] / (hp / host_s)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--budget-s", type=float, default=60.0)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-pairs", type=int, default=2048)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-commit", default=None)
    ap.add_argument("--out", default=os.path.join(provenance.ROOT, "profiles", "stem_grad.json"))
    a = ap.parse_args()
    ctx = ska.Context(0)
    doc = dict(device="MI355X (gfx950)", kind="SK_SU_STEM", calls=a.calls, warmup=a.warmup,
               provenance=dict(source_hash=provenance.source_hash()),
               note="gpu_ms: the call's GPU span (prep kernel and pair kernel); forward_gram: sk_gram with "
                    "SK_SU_STEM over the same set (the register-class kernel, the floor); host: "
                    "sk_stem_gradients_host, wall clock")
    small = measure(ctx, min(256, a.n), a.length, a, host=True)
    doc["n256"] = small
    if a.n > 256:
        pairs = a.n * (a.n + 1) // 2
        projected = pairs / small["pairs_per_s"]
        doc["projected_s_for_n"] = dict(n=a.n, pairs=pairs, seconds=projected, budget_s=a.budget_s)
        if projected <= a.budget_s:
            doc["n%d" % a.n] = measure(ctx, a.n, a.length, a, host=False)
            doc["headline"] = "n%d" % a.n
        else:
            doc["headline"] = "n256"
            doc["headline_note"] = ("the upper triangle of %d examples projects %.0f s per call, over the %.0f s "
                                    "budget: the 256-example figures stand" % (a.n, projected, a.budget_s))
    else:
        doc["headline"] = "n256"
    for key, path in (("bench_parent", a.bench_parent), ("bench_commit", a.bench_commit)):
        if path:
            with open(path) as f:
                lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
            doc[key] = json.loads(lines[-1])
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[doc["headline"]][k] for k in ("examples", "pairs", "median_ms", "pairs_per_s",
                                                            "gradient_over_forward")}))


if __name__ == "__main__":
    main()
