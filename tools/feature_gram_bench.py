#!/usr/bin/env python3
"""The feature-vector Grams (sk_feature_gram, csrc/kernels/feature_gram.hip)
on one MI355X against the host path on 16 threads.

Shapes: 2,048 examples x 512 columns dense, and 4,096 examples at 2 % density
over 4,096 used columns (labels: the sign of the example's sum, so the folds
are learnable).  Timed, each the median of --calls calls after --warmup
warm-ups (the dot matrix of a fresh copy of the set each time):
  feat_dot     the ordered FP64 dot matrix: GPU span of its launch (HIP events,
               Context.last_launch_ms) and the wall time of the call that
               computes it (densify, upload, kernel)
  feat_apply   per kernel, with D resident: GPU span of the launch and the wall
               time of sk_feature_gram (kernel, download of K and G)
  step         wall time of one Context.feature_auc_objective step (5 folds)
               with D resident, and of its parts
  host         sk_feature_dots_host and sk_feature_gram_host on --threads
  torch.matmul FP64 X X^T on the same card, for scale only: an unordered sum
               (MFMA, split sums), so it shows the price of the ordered one
The GPU's D is compared with the host's bit for bit.  feat_dot issues two FP64
vector instructions per term (multiply, add; n^2 d terms, or n (n + T) d / 2
for the symmetric case's tiles): `valu_frac` is that count over the card's
FP64 vector issue rate (256 CUs x 64 lanes per clock x 2.4 GHz = 39.3e12
instructions/s, half the 78.6 TFLOPS an FMA counts twice).  feat_apply moves
(2 + P) n^2 doubles: `hbm_frac` is that over 8 TB/s.  Writes one JSON document
(--out); no pass/fail threshold."""
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

FP64_ISSUE = 256 * 64 * 2.4e9
HBM = 8e12


def make(n, d, density, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(-1024, 1025, size=(n, d)) / 512.0
    if density < 1.0:
        X[rng.random((n, d)) >= density] = 0.0
    X[:, 0] = np.where(X[:, 0] == 0, 0.25, X[:, 0])  # no empty example
    X[0, :] = np.where(X[0, :] == 0, 0.5, X[0, :])   # every column used
    y = np.where(X.sum(axis=1) >= 0, 1, -1)
    return X, y


def med(f, calls, warmup):
    ts = []
    for k in range(calls + warmup):
        t, extra = f()
        if k >= warmup:
            ts.append((t, extra))
    return statistics.median(t for t, _ in ts), statistics.median(e for _, e in ts)


def run_shape(ctx, name, n, d, density, a):
    X, y = make(n, d, density, 0xBE7C + n)
    T = ska.feature_gram_shape()["tile"]
    res = dict(name=name, n=n, d=d, density=density)

    def fresh_dots():
        fs = ska.FeatureSet.from_dense(X, y)
        t0 = time.perf_counter()
        ska.feature_dots(fs, ctx=ctx)
        t = time.perf_counter() - t0
        ms = ctx.last_launch_ms()
        assert ms["launches"] == 1
        fs.close()
        return t * 1e3, ms["ms_sum"]

    wall, span = med(fresh_dots, a.calls, a.warmup)
    terms = n * (n + T) / 2 * d  # the tiles with tile_i <= tile_j, whole
    res["feat_dot"] = dict(wall_ms=wall, gpu_ms=span, terms=terms, terms_per_s=terms / (span * 1e-3),
                           valu_frac=2 * terms / (span * 1e-3) / FP64_ISSUE)
    fs = ska.FeatureSet.from_dense(X, y)
    assert fs.shape[:2] == (n, d)
    D = ska.feature_dots(fs, ctx=ctx)
    t0 = time.perf_counter()
    Dh = ska.feature_dots(fs, n_threads=a.threads)
    res["host_dots_ms"] = (time.perf_counter() - t0) * 1e3
    res["dots_bit_identical"] = bool(np.array_equal(D.view(np.uint64), Dh.view(np.uint64)))
    kernels = dict(rbf=ska.RBFKernel(1.0 / d), poly=ska.PolyKernel(3, 1.0 / d, 1.0), sigmoid=ska.SigmoidKernel(1.0 / d, 0.0))
    res["feat_apply"] = {}
    for kname, kern in kernels.items():
        def apply():
            t0 = time.perf_counter()
            ska.feature_gram(fs, kern, ctx=ctx)
            t = time.perf_counter() - t0
            ms = ctx.last_launch_ms()
            assert ms["launches"] == 1
            return t * 1e3, ms["ms_sum"]
        wall, span = med(apply, a.calls, a.warmup)
        P = len(kern.params)
        t0 = time.perf_counter()
        Kh, Gh = ska.feature_gram(fs, kern, n_threads=a.threads)
        host = (time.perf_counter() - t0) * 1e3
        Kg, Gg = ska.feature_gram(fs, kern, ctx=ctx)
        scale = lambda r: np.where(r != 0, np.abs(r), np.abs(r).max())
        res["feat_apply"][kname] = dict(
            wall_ms=wall, gpu_ms=span, bytes=(2 + P) * n * n * 8, hbm_frac=(2 + P) * n * n * 8 / (span * 1e-3) / HBM,
            host_gram_ms=host, max_rel_dev_K=float(np.max(np.abs(Kg - Kh) / scale(Kh))),
            max_rel_dev_G=float(max(np.max(np.abs(g - h) / scale(h)) for g, h in zip(Gg, Gh))))
    # one optimizer step with D resident, and its parts
    kern = kernels["rbf"]

    def step():
        t0 = time.perf_counter()
        ctx.feature_auc_objective(fs, kern, a.folds, 1.0)
        return (time.perf_counter() - t0) * 1e3, 0.0

    res["step"] = dict(folds=a.folds, kernel="rbf", wall_ms=med(step, a.calls, a.warmup)[0])
    K, G = ska.feature_gram(fs, kern, ctx=ctx)
    t0 = time.perf_counter()
    ska.auc_objective(K, G, fs.labels, a.folds, 1.0, ctx=ctx)
    res["step"]["auc_objective_ms"] = (time.perf_counter() - t0) * 1e3
    res["step"]["feature_gram_ms"] = res["feat_apply"]["rbf"]["wall_ms"]
    try:
        import torch
        Xt = torch.tensor(X, dtype=torch.float64, device="cuda:0")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for k in range(a.calls + a.warmup):
            ev[0].record()
            torch.matmul(Xt, Xt.T)
            ev[1].record()
            torch.cuda.synchronize()
            if k >= a.warmup:
                ts.append(ev[0].elapsed_time(ev[1]))
        res["torch_matmul_fp64_ms"] = statistics.median(ts)
    except Exception as e:  # for scale only
        res["torch_matmul_fp64_ms"] = None
        res["torch_error"] = repr(e)
    fs.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_gram.json"))
    a = ap.parse_args()
    ctx = ska.Context(0)
    doc = dict(tool="tools/feature_gram_bench.py", calls=a.calls, warmup=a.warmup, threads=a.threads,
               shape=ska.feature_gram_shape(), fp64_issue_per_s=FP64_ISSUE, hbm_bytes_per_s=HBM,
               shapes=[run_shape(ctx, "2048 x 512 dense", 2048, 512, 1.0, a),
                       run_shape(ctx, "4096 x 4096 at 2 %", 4096, 4096, 0.02, a)])
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
