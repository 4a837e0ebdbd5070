#!/usr/bin/env python3
"""Throughput of the protein local-alignment kernels (SK_AA_LA / SK_AA_LA_SW,
csrc/kernels/la_protein.hip) on one MI355X, beside the nearest RNA kernel.

  code path     Gram of --n random single proteins, lengths uniform in 150-450
  profile path  Gram of --n-aln four-row alignments of about 300 columns
  comparison    SK_LA (BPLAKernel noBP, bpla.hip's fast path: one exp per cell)
                on RNA single sequences of the same lengths, alternating with
                the protein calls in the same run

Each figure is the median of --calls calls after --warmup warm-ups, from the
call's GPU span (Context.last_timing).  Writes one JSON document (--out).
--counters runs each code-path kernel once and nothing else, for a
counter-only profiler run around this script.

--gradients measures the gradient kernels instead (sk_la_protein_gradients,
csrc/kernels/la_protein_grad.hip):

  code path     upper triangle of --n-grad (1,024) single proteins of length
                200: 524,800 pairs
  profile path  upper triangle of --n-aln (256) three-row alignments of about
                200 columns
  beside each   sk_gram with SK_AA_LA over the same pairs (the forward kernel
                alone: the floor) and the host path on --host-threads (16)
                threads over the first --host-pairs pairs of the same list"""
import argparse
import json
import statistics
import sys
import os

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stem_kernel_amd as ska  # noqa: E402

AA20 = np.array(list("ARNDCQEGHILKMFPSTWYV"))
RNA = np.array(list("ACGU"))


def random_rows(rng, alphabet, lengths):
    return ["".join(alphabet[rng.integers(0, len(alphabet), int(n))]) for n in lengths]


def alignments(rng, n, cols=300, rows=4):
    out = []
    for _ in range(n):
        L = int(rng.integers(cols - 20, cols + 21))
        base = rng.integers(0, 20, L)
        al = []
        for _r in range(rows):
            r = base.copy()
            mut = rng.random(L) < 0.25
            r[mut] = rng.integers(0, 20, int(mut.sum()))
            s = AA20[r]
            s[rng.random(L) < 0.05] = "-"
            al.append("".join(s))
        out.append(al)
    return out


def measure(ctx, jobs, calls, warmup):
    """jobs: name -> (dataset, kernel); the calls alternate between the jobs."""
    ms = {k: [] for k in jobs}
    cells = {}
    for it in range(warmup + calls):
        for name, (ds, kern) in jobs.items():
            ctx.gram(ds, kern)
            t = ctx.last_timing()
            cells[name] = t["cells"]
            if it >= warmup:
                ms[name].append(t["stem_ms"])
    out = {}
    for name, (ds, _k) in jobs.items():
        med = statistics.median(ms[name])
        pairs = len(ds) * (len(ds) + 1) // 2
        out[name] = dict(examples=len(ds), pairs=pairs, cells=cells[name], gpu_ms=ms[name], median_ms=med,
                         pairs_per_s=pairs / (med * 1e-3), cells_per_s=cells[name] / (med * 1e-3))
    return out


def gradients(ctx, a, rng):
    """The --gradients document: per path the GPU span of the gradient call,
    the forward Gram's over the same pairs and the host path over a subset."""
    import time

    from stem_kernel_amd import provenance
    code = ska.Dataset()
    for s in random_rows(rng, AA20, [200] * a.n_grad):
        code.add_protein("+1", [s])
    prof = ska.Dataset()
    for al in alignments(rng, a.n_aln, cols=200, rows=3):
        prof.add_protein("+1", al)
    kern = ska.LAKernel()
    res = dict(device="MI355X (gfx950)", calls=a.calls, warmup=a.warmup, provenance=provenance.stamp(),
               limits=ska.la_grad_shape(),
               b_bytes_written_per_cell=24, b_bytes_read_per_cell=24,
               note="gpu_ms: the call's GPU span (both passes of every pair); forward_gram: sk_gram with SK_AA_LA "
                    "over the same pairs (the floor); host: sk_la_protein_gradients_host, wall clock")
    for name, ds in (("code", code), ("profile", prof)):
        n = len(ds)
        x, y = (v.astype(np.int32) for v in np.triu_indices(n))
        g_ms, f_ms = [], []
        cells = 0.0
        for it in range(a.warmup + a.calls):
            ctx.la_gradients(ds, kern, x, y)
            t = ctx.last_timing()
            ran = ctx.last_la_protein_grad()
            cells = t["cells"]
            if it >= a.warmup:
                g_ms.append(t["stem_ms"])
            ctx.gram(ds, kern)
            if it >= a.warmup:
                f_ms.append(ctx.last_timing()["stem_ms"])
        hp = min(a.host_pairs, x.size)
        t0 = time.perf_counter()
        ska.la_gradients(ds, kern, x[:hp], y[:hp], n_threads=a.host_threads)
        host_s = time.perf_counter() - t0
        gm, fm = statistics.median(g_ms), statistics.median(f_ms)
        res[name] = dict(examples=n, pairs=int(x.size), cells=cells, kernels=ran, gpu_ms=g_ms, median_ms=gm,
                         pairs_per_s=x.size / (gm * 1e-3), cells_per_s=cells / (gm * 1e-3),
                         b_bytes_written=24.0 * cells,
                         forward_gram=dict(gpu_ms=f_ms, median_ms=fm, pairs_per_s=x.size / (fm * 1e-3)),
                         gradient_over_forward=gm / fm,
                         host=dict(threads=a.host_threads, pairs=int(hp), subset="the first pairs of the same list",
                                   seconds=host_s, pairs_per_s=hp / host_s),
                         gpu_over_host_pairs_per_s=(x.size / (gm * 1e-3)) / (hp / host_s))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--n-aln", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--counters", action="store_true")
    ap.add_argument("--gradients", action="store_true")
    ap.add_argument("--n-grad", type=int, default=1024)
    ap.add_argument("--host-pairs", type=int, default=2048)
    ap.add_argument("--host-threads", type=int, default=16)
    a = ap.parse_args()
    rng = np.random.default_rng(0x1A9E57)
    if a.gradients:
        text = json.dumps(gradients(ska.Context(0), a, rng), indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    lengths = rng.integers(150, 451, a.n)
    prot = ska.Dataset()
    for s in random_rows(rng, AA20, lengths):
        prot.add_protein("+1", [s])
    ctx = ska.Context(0)
    if a.counters:
        for sw in (False, True):
            ctx.gram(prot, ska.LAKernel(SW=sw))
            print(json.dumps(dict(kernel="code", SW=sw, **ctx.last_timing())), flush=True)
        return
    rna = ska.Dataset()
    for s in random_rows(rng, RNA, lengths):
        rna.add("+1", [s], use_bp=False)
    aln = ska.Dataset()
    for al in alignments(rng, a.n_aln):
        aln.add_protein("+1", al)
    res = dict(device="MI355X (gfx950)", calls=a.calls, warmup=a.warmup,
               lengths=dict(min=int(lengths.min()), max=int(lengths.max()), mean=float(lengths.mean())))
    res.update(measure(ctx, {"aa_la_code": (prot, ska.LAKernel()), "rna_la": (rna, ska.BPLAKernel(noBP=True)),
                             "aa_la_sw_code": (prot, ska.LAKernel(SW=True)),
                             "rna_la_sw": (rna, ska.BPLAKernel(noBP=True, SW=True))}, a.calls, a.warmup))
    res.update(measure(ctx, {"aa_la_profile": (aln, ska.LAKernel()), "aa_la_sw_profile": (aln, ska.LAKernel(SW=True))},
                       a.calls, a.warmup))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
