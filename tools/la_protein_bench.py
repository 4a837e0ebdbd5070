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
counter-only profiler run around this script."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--n-aln", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--counters", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0x1A9E57)
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
