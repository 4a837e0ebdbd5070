"""Call time of the stochastic structure sampler (sk_fold_sample, bpp only)
against the McCaskill fold (sk_fold_mccaskill) of the same batch, on one GPU:
the median of `runs` timed calls after `warm` warm-up calls each, the two
alternating.  A second series at other sample counts separates the part of
the call that does not grow with N (inside pass, copies) from the walks.

    python tools/fold_sample_bench.py [n_seqs] [length] [n_samples] [out.json]
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stem_kernel_amd as ska  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    ns = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    out = sys.argv[4] if len(sys.argv) > 4 else None
    warm, runs = 2, 5
    seqs = ska.random_sequences(n, L, 0x5EED0002)
    ctx = ska.Context(0)

    def timed(fn):  # both calls end in a stream synchronise
        t = time.perf_counter()
        fn()
        return time.perf_counter() - t

    calls = {"fold": lambda: ctx.fold(seqs), "sample": lambda: ctx.fold_sample(seqs, ns, seed=1)}
    times = {k: [] for k in calls}
    for r in range(warm + runs):
        for k, fn in calls.items():
            t = timed(fn)
            if r >= warm:
                times[k].append(t)
    fold_s = statistics.median(times["fold"])
    sample_s = statistics.median(times["sample"])
    series = {}
    for m in (ns // 10, ns * 4):
        if m < 1:
            continue
        ctx.fold_sample(seqs, m, seed=1)
        series[m] = statistics.median(timed(lambda: ctx.fold_sample(seqs, m, seed=1)) for _ in range(3))
    res = {"metric": f"fold_sample vs fold, {n} random sequences of L={L}, N={ns}, bpp only",
           "n_seqs": n, "length": L, "n_samples": ns, "warmups": warm, "runs": runs,
           "fold_s": fold_s, "fold_s_all": times["fold"],
           "fold_sample_s": sample_s, "fold_sample_s_all": times["sample"],
           "samples_per_s": n * ns / sample_s, "ratio_sample_over_fold": sample_s / fold_s,
           "fold_sample_s_by_n_samples": {str(k): v for k, v in series.items()}}
    if len(series) == 2:
        (a, ta), (b, tb) = sorted(series.items())
        per = (tb - ta) / ((b - a) * n)
        res["walk_s_per_sample"] = per
        res["fixed_s"] = ta - per * a * n
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
