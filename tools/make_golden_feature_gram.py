#!/usr/bin/env python3
"""Generate tests/golden/features_small.txt, tests/golden/feature_gram.json and
tests/golden/feature_gram.npz from the reference's own feature-vector kernels.

The feature file is made here (deterministic); every recorded value comes from
tests/cpp/feature_gram_ref_harness.cpp, which includes the reference's
optimizer/rbf_kernel.cpp, poly_kernel.cpp or sigmoid_kernel.cpp in place (one
binary per kernel) and is compiled into a temporary directory over the Boost
stand-ins (tests/cpp/feature_standin, oracle/ref_shim/standin).  Nothing
compiled from the reference is kept.

    python tools/make_golden_feature_gram.py /path/to/reference [out-dir]

The file exercises every case the reader must agree with read_data on: "+1"
labels, a blank line (label 0, no features), trailing blanks and a carriage
return, exponents, explicit zero values (of both signs), a far-apart index,
and a last line without a newline.  The JSON holds the labels and the vectors
read_data produced (values as hex floats) and each case's kernel, degree and
parameters; the .npz holds, as float64 arrays parsed from the harness's hex
floats (the same bits; 17 matrices as text would be 370 KB), the upper
triangles (i <= j, row by row) of dot() as "D" and, per case c, of K and the
gradient matrices as "K<c>" and "G<c>" (P rows) -- two parameter settings per
kernel, a polynomial degree 1 and an even degree with negative
t = gamma d + coef0 among them.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, COLS = 44, 24
# (kernel, SK_FEAT_KERNEL, degree, params)
SETTINGS = [("rbf", 0, 0, [0.5]), ("rbf", 0, 0, [0.01]),
            ("poly", 1, 1, [0.7, 0.3]), ("poly", 1, 4, [0.5, -1.0]),
            ("sigmoid", 2, 0, [0.05, 0.1]), ("sigmoid", 2, 0, [0.3, -0.5])]


def feature_text():
    rng = np.random.default_rng(0x5A17F001)
    lines = []
    for i in range(N):
        if i == 5:
            lines.append("")  # label 0, no features
            continue
        label = "+1" if i % 3 == 0 else ("1" if i % 3 == 1 and i % 2 else "-1")
        cols = sorted(rng.choice(np.arange(1, COLS + 1), size=int(rng.integers(3, 15)), replace=False).tolist())
        toks = []
        for c in cols:
            v = round(float(rng.uniform(-2.0, 2.0)), 3)
            style = int(rng.integers(0, 4))
            toks.append(f"{c}:{v:.3e}" if style == 0 else f"{c}:{v:.2E}" if style == 1 else f"{c}:{v!r}")
        if i == 7:
            toks.append("100000:1.5")  # far apart: costs one compacted column
        if i == 9:
            toks.insert(0, "0:0")      # explicit zeros, index 0 included
            toks.append("30:-0.0")
        if i == 11:
            toks = ["2147483646:2.5e-1"]  # the largest index but one
        line = label + " " + " ".join(toks)
        if i % 7 == 2:
            line += "  \t "
        if i == 13:
            line += "\r"
        if i == 17:
            line = "  " + line.replace(" ", "   ", 2)
        lines.append(line)
    return "\n".join(lines)  # no newline after the last line


def build(ref, workdir, k):
    exe = os.path.join(workdir, f"feature_gram_ref_harness_{k}")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-w", f"-DSK_FEAT_KERNEL={k}",
                    "-I", os.path.join(ROOT, "tests", "cpp", "feature_standin"),
                    "-I", os.path.join(ROOT, "oracle", "ref_shim", "standin"), "-I", ref,
                    "-I", os.path.join(ref, "optimizer"),
                    os.path.join(ROOT, "tests", "cpp", "feature_gram_ref_harness.cpp"), "-o", exe],
                   check=True, cwd=workdir)
    return exe


def run(exe, path, degree, params):
    out = subprocess.run([exe, path, str(degree)] + [float(p).hex() for p in params], check=True,
                         capture_output=True, text=True).stdout.split("\n")
    res = dict(V=[])
    for line in out:
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "V":
            res["V"].append([[int(t.split(":")[0]), t.split(":")[1]] for t in tok[1:]])
        else:
            res[tok[0]] = tok[1:]
    return res


def generate(ref, outdir):
    text = feature_text()
    path = os.path.join(outdir, "features_small.txt")
    with open(path, "w", newline="") as f:
        f.write(text)
    golden = dict(file="features_small.txt", matrices="feature_gram.npz", kernels=[])
    arrays = {}
    unhex = lambda hexes: np.array([float.fromhex(v) for v in hexes], dtype=np.float64)
    with tempfile.TemporaryDirectory() as d:
        exes = {}
        for name, k, degree, params in SETTINGS:
            if k not in exes:
                exes[k] = build(ref, d, k)
            r = run(exes[k], path, degree, params)
            labels, vectors = [int(v) for v in r["L"]], r["V"]
            n = len(labels)
            assert n == N and len(vectors) == n and len(r["D"]) == n * (n + 1) // 2
            if "labels" not in golden:
                golden.update(labels=labels, vectors=vectors, D=r["D"])
            assert (golden["labels"], golden["vectors"], golden["D"]) == (labels, vectors, r["D"])
            G = [r["G0"]] + ([r["G1"]] if len(params) > 1 else [])
            assert all(len(m) == len(r["D"]) for m in [r["K"]] + G)
            c = len(golden["kernels"])
            golden["kernels"].append(dict(kernel=name, degree=degree, params=[float(p).hex() for p in params]))
            arrays[f"K{c}"] = unhex(r["K"])
            arrays[f"G{c}"] = np.stack([unhex(m) for m in G])
    # the cases the header promises
    arrays["D"] = unhex(golden.pop("D"))
    ts = [float.fromhex(p["params"][0]) * dv + float.fromhex(p["params"][1])
          for p in golden["kernels"] if p["kernel"] == "poly" and p["degree"] % 2 == 0 for dv in arrays["D"]]
    assert min(ts) < 0 < max(ts)
    assert any(p["kernel"] == "poly" and p["degree"] == 1 for p in golden["kernels"])
    with open(os.path.join(outdir, "feature_gram.json"), "w") as f:
        json.dump(golden, f, separators=(",", ":"))
        f.write("\n")
    np.savez_compressed(os.path.join(outdir, "feature_gram.npz"), **arrays)
    return path


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden")
    print(generate(sys.argv[1], out))
