#!/usr/bin/env python3
"""Throughput of the palindrome kernel (SK_SIMPAL, csrc/kernels/simpal.hip)
on one MI355X.

  set 1   Gram of --n random sequences of --len letters (1024 x 200)
  set 2   Gram of --n2 random sequences of --len2 letters (256 x 400)

Base-pairing probabilities from sk_fold_synthetic without GU pairs, the CLI's
default parameters (seed_length 3, min_loop 3, max_dist 300, tolerance 1).
Each figure is the median of --calls calls after --warmup warm-ups: pairs/s
and terms/s (the sum of |P_x| |P_y| over the call) over the call's wall time
(host planning, upload of the pair lists, kernel, download) and over its GPU
span (Context.last_timing), and the mean |P|.  --check N also compares the
Gram of the first N examples of each set with the numpy restatement
(tests/simpal_ref.py) and reports the largest relative deviation.  Writes one
JSON document (--out).  --once runs each Gram once and nothing else, for a
counter-only profiler run around this script."""
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


def build(n, length, seed):
    seqs = ska.random_sequences(n, length, seed)
    ds = ska.Dataset()
    for s in seqs:
        ds.add_palindromes("+1", s)  # fold(seq.lower(), no_gu=True)
    sizes = np.array([len(ds.palindromes(i)[0]) for i in range(n)])
    return ds, sizes


def measure(ctx, ds, sizes, calls, warmup):
    kern = ska.SimpalKernel()
    n = len(ds)
    pairs = n * (n + 1) // 2
    wall, gpu, terms = [], [], 0.0
    for it in range(warmup + calls):
        t0 = time.perf_counter()
        ctx.gram(ds, kern)
        t1 = time.perf_counter()
        t = ctx.last_timing()
        terms = t["cells"]
        if it >= warmup:
            wall.append((t1 - t0) * 1e3)
            gpu.append(t["stem_ms"])
    iu, ju = np.triu_indices(n)
    assert terms == float((sizes[iu].astype(np.float64) * sizes[ju]).sum())
    mw, mg = statistics.median(wall), statistics.median(gpu)
    return dict(examples=n, pairs=pairs, terms=terms, mean_entries=float(sizes.mean()),
                min_entries=int(sizes.min()), max_entries=int(sizes.max()),
                wall_ms=wall, gpu_ms=gpu, median_wall_ms=mw, median_gpu_ms=mg,
                pairs_per_s_wall=pairs / (mw * 1e-3), terms_per_s_wall=terms / (mw * 1e-3),
                pairs_per_s_gpu=pairs / (mg * 1e-3), terms_per_s_gpu=terms / (mg * 1e-3))


def deviation(ctx, ds, m):
    from tests import simpal_ref
    sub = ska.Dataset()
    for i in range(m):
        ska.lib().sk_dataset_add_copy(sub.handle, ds.handle, i)
    ent = [sub.palindromes(i) for i in range(m)]
    got = ctx.gram(sub, ska.SimpalKernel())
    ref = simpal_ref.gram(ent, 1)
    nz = ref != 0
    assert np.array_equal(got[~nz], ref[~nz])
    return float(np.max(np.abs(got[nz] - ref[nz]) / ref[nz])) if nz.any() else 0.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--len", type=int, default=200)
    ap.add_argument("--n2", type=int, default=256)
    ap.add_argument("--len2", type=int, default=400)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=32)
    ap.add_argument("--out", default="")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    sets = {f"n{a.n}_len{a.len}": build(a.n, a.len, 0x51A9A100), f"n{a.n2}_len{a.len2}": build(a.n2, a.len2, 0x51A9A101)}
    ctx = ska.Context(0)
    if a.once:
        for name, (ds, _s) in sets.items():
            ctx.gram(ds, ska.SimpalKernel())
            print(json.dumps(dict(set=name, **ctx.last_timing())), flush=True)
        return
    res = dict(device="MI355X (gfx950)", calls=a.calls, warmup=a.warmup, shape=dict(zip(("y_tile", "x_block"), ska.simpal_shape())))
    for name, (ds, sizes) in sets.items():
        res[name] = measure(ctx, ds, sizes, a.calls, a.warmup)
        if a.check > 0:
            res[name]["max_rel_deviation_vs_restatement"] = deviation(ctx, ds, min(a.check, len(ds)))
            res[name]["deviation_examples"] = min(a.check, len(ds))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
