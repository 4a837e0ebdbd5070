"""Call time of the consensus fold (sk_fold_alignment) of `n_aln` alignments
of `length` columns at several row counts S, against the McCaskill fold
(sk_fold_mccaskill) of n_aln sequences (one fold per alignment) and of
n_aln * S sequences (the per-row folds the averaged path costs), on one GPU:
the median of `runs` timed calls after `warm` warm-up calls each, the calls
of one S alternating.

    python tools/fold_alignment_bench.py [n_aln] [length] [out.json]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stem_kernel_amd as ska  # noqa: E402


def alignments(n_aln, length, S, seed):
    """S gap-free rows per alignment: a random sequence and copies with a
    tenth of the columns changed (so every row folds at the same cost)."""
    rng = np.random.default_rng(seed)
    base = ska.random_sequences(n_aln, length, 0x5EED0002)
    alns = []
    for s in base:
        rows = [s]
        for _ in range(S - 1):
            r = list(s)
            for k in rng.choice(length, max(length // 10, 1), replace=False):
                r[k] = "ACGU"[int(rng.integers(0, 4))]
            rows.append("".join(r))
        alns.append(rows)
    return alns


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    out = sys.argv[3] if len(sys.argv) > 3 else None
    warm, runs = 2, 5
    ctx = ska.Context(0)

    def timed(fn):  # every call ends in a stream synchronise
        t = time.perf_counter()
        fn()
        return time.perf_counter() - t

    res = {"metric": f"fold_alignment of {n} alignments of {L} columns vs fold of {n} and of {n} * S sequences",
           "n_aln": n, "length": L, "warmups": warm, "runs": runs, "by_rows": {}}
    for S in (1, 5, 20):
        alns = alignments(n, L, S, 7 + S)
        firsts = [a[0] for a in alns]
        rows = [r for a in alns for r in a]
        calls = {"fold_alignment": lambda: ctx.fold_alignment(alns),
                 "fold_one_per_alignment": lambda: ctx.fold(firsts),
                 "fold_every_row": lambda: ctx.fold(rows)}
        times = {k: [] for k in calls}
        for r in range(warm + runs):
            for k, fn in calls.items():
                t = timed(fn)
                if r >= warm:
                    times[k].append(t)
        med = {k: statistics.median(v) for k, v in times.items()}
        res["by_rows"][str(S)] = {
            "fold_alignment_s": med["fold_alignment"], "fold_alignment_s_all": times["fold_alignment"],
            "fold_one_per_alignment_s": med["fold_one_per_alignment"],
            "fold_one_per_alignment_s_all": times["fold_one_per_alignment"],
            "fold_every_row_s": med["fold_every_row"], "fold_every_row_s_all": times["fold_every_row"],
            "ratio_to_one_fold": med["fold_alignment"] / med["fold_one_per_alignment"],
            "ratio_to_row_folds": med["fold_alignment"] / med["fold_every_row"]}
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
