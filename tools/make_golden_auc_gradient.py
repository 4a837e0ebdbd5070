#!/usr/bin/env python3
"""Generate tests/golden/auc_gradient.json from the reference's own gradient code.

The matrices and problems are made here (deterministic); every recorded value
comes from tests/cpp/auc_gradient_ref_harness.cpp, which includes the
reference's optimizer/gradient.cpp, libsvm/solver.cpp and libsvm/qmatrix.cpp
in place and is compiled into a temporary directory over the Boost stand-ins
(tests/cpp/ublas_standin, oracle/ref_shim/standin).  Nothing compiled from
the reference is kept.

    python tools/make_golden_auc_gradient.py /path/to/reference [out.json]

Integer Grams (tests/svm_ref.int_gram) are stored as their seeds; the 40 x 40
RBF Gram of tests/golden/svm_train.json and its gradient matrix -D K (the
derivative with respect to gamma of K = exp(-gamma D)) are stored as hex
floats.  Natural problems (a fold trained by the reference's Solver without
shrinking, then its own svm_predict) record alpha, rho and the decision
values the harness produced; crafted ones record the ones given.  Every
problem records f and delta (compute_delta), n_free, n_bound, the conjugate
gradient's product count, d_u, cg and fg (what the engine must reproduce),
and for natural problems compute()'s f, cg, fg with its hardcoded
shrinking = 1 (for the record in DESIGN.md; not asserted).
"""
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAMMA = 0.5


def matrices():
    from tests import svm_ref
    ms = [dict(kind="int", seed=0x5A17A101, n=300, d=6, shift=2, indef=0, dup=0)]
    ms += [dict(kind="int", seed=0x5A17C000 + k, n=300, d=6, shift=2, indef=0, dup=0) for k in (1, 2, 3)]
    # the RBF Gram of the SVM fixture (tools/make_golden_svm_train.py) and dK/dgamma
    r = svm_ref.splitmix64_stream(0x5A17A104, 80)
    pts = [((int(r[2 * k]) % 2001) / 500.0 - 2.0, (int(r[2 * k + 1]) % 2001) / 500.0 - 2.0) for k in range(40)]
    kv, gv = [], []
    for a in pts:
        for b in pts:
            D = (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2
            k = math.exp(-GAMMA * D)
            kv.append(k.hex())
            gv.append((-D * k).hex())
    labels = [1 if a[0] ** 2 + a[1] ** 2 < 2.0 else -1 for a in pts]
    labels[0], labels[1] = 1, -1
    ms.append(dict(kind="stored", n=40, values=kv, labels=labels))
    ms.append(dict(kind="stored", n=40, values=gv))
    ms.append(dict(kind="int", seed=0x5A17C010, n=60, d=5, shift=1, indef=0, dup=0, asym=1))
    ms.append(dict(kind="int", seed=0x5A17C011, n=60, d=5, shift=1, indef=0, dup=0, asym=1))
    return ms


K300, G300, KRBF, GRBF, KASYM, GASYM = 0, [1, 2, 3], 4, [5], 6, [7]


def problems(mats):
    from tests import auc_ref, svm_ref
    ps = []

    def natural(name, k, g, train, test, C):
        ps.append(dict(name=name, k=k, g=list(g), train=[int(t) for t in train], test=[int(t) for t in test],
                       C=C, natural=1, eps=1e-3))

    def craft(name, k, g, train, test, C, n_free, n_bound, seed):
        alpha, rho, dec = auc_ref.crafted(seed, train, test, C, n_free, n_bound)
        ps.append(dict(name=name, k=k, g=list(g), train=[int(t) for t in train], test=[int(t) for t in test],
                       C=C, natural=0, eps=1e-3, alpha=[float(a).hex() for a in alpha], rho=float(rho).hex(),
                       dec=[float(v).hex() for v in dec]))

    for C in (1.0, 2.0 ** -3):
        for cv in range(5):
            tr, ts = svm_ref.split(300, 5, cv)
            natural(f"int300 C={C:g} cv={cv}", K300, G300, tr, ts, C)
    for C in (1.0, 64.0):
        for cv in range(5):
            tr, ts = svm_ref.split(40, 5, cv)
            natural(f"rbf C={C:g} cv={cv}", KRBF, GRBF, tr, ts, C)
    tr, ts = svm_ref.split(300, 5, 0)
    for nf in (0, 1, 2, 10):
        craft(f"crafted n_free={nf}", K300, G300, tr, ts, 2.0, nf, 17, 0xA0C0 + nf)
    craft("crafted all at the bound", K300, G300, tr, ts, 0.5, 0, len(tr), 0xA0D0)
    craft("crafted no support vector", K300, G300, tr, ts, 0.5, 0, 0, 0xA0D1)
    y300 = mats[K300][1]
    craft("one-class test list", K300, G300, tr, [int(t) for t in ts if y300[t] > 0][:12], 1.0, 6, 9, 0xA0D2)
    craft("n_params = 0", K300, [], tr, ts, 1.0, 8, 11, 0xA0D3)
    perm = [(k * 37 + 11) % 150 for k in range(150)]  # 37 and 150 are coprime
    craft("permuted training list", K300, G300, perm, list(range(150, 200)), 1.0, 9, 20, 0xA0D4)
    craft("non-symmetric K", KASYM, GASYM, list(range(0, 45)), list(range(45, 60)), 1.0, 7, 5, 0xA0D5)
    return ps


def build_harness(ref, workdir):
    """Compile the harness (which includes the reference's sources) into workdir."""
    exe = os.path.join(workdir, "auc_gradient_ref_harness")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-w", "-I", os.path.join(ROOT, "tests", "cpp", "ublas_standin"),
                    "-I", os.path.join(ROOT, "oracle", "ref_shim", "standin"), "-I", ref,
                    "-I", os.path.join(ref, "libsvm"),
                    os.path.join(ROOT, "tests", "cpp", "auc_gradient_ref_harness.cpp"), "-o", exe],
                   check=True, cwd=workdir)
    return exe


def run_harness(exe, workdir, mats, ps):
    path = os.path.join(workdir, "auc_input.txt")
    with open(path, "w") as f:
        f.write(f"{len(mats)}\n")
        for M, _ in mats:
            f.write(f"{M.shape[0]}\n" + " ".join(float(v).hex() for v in M.reshape(-1)) + "\n")
        f.write(f"{len(ps)}\n")
        for p in ps:
            y = mats[p["k"]][1]
            f.write(f"{p['k']} {len(p['g'])} " + " ".join(map(str, p["g"])) +
                    f" {len(p['train'])} {len(p['test'])} {float(p['C']).hex()} {p['natural']} "
                    f"{float(p['eps']).hex()}\n")
            f.write(" ".join(str(int(v)) for v in y) + "\n")
            f.write(" ".join(map(str, p["train"])) + "\n" + " ".join(map(str, p["test"])) + "\n")
            if not p["natural"]:
                f.write(" ".join(p["alpha"]) + "\n" + p["rho"] + "\n" + " ".join(p["dec"]) + "\n")
    out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split("\n")
    pos = 0

    def line(tag):
        nonlocal pos
        tok = out[pos].split()
        pos += 1
        assert tok[0] == tag, (tag, tok[:3])
        return tok[1:]

    for p in ps:
        l, m, q = len(p["train"]), len(p["test"]), len(p["g"])
        a = line("A")
        assert len(a) == l + 1 + m
        if not p["natural"]:
            given = p["alpha"] + [p["rho"]] + p["dec"]
            assert [float.fromhex(v) for v in a] == [float.fromhex(v) for v in given]
        p["alpha"], p["rho"], p["dec"] = a[:l], a[l], a[l + 1:]
        fd = line("F")
        p["f"], p["delta"] = fd[0], fd[1:]
        assert len(p["delta"]) == m
        s = line("S")
        p["n_free"], p["n_bound"], p["cg_iterations"] = int(s[0]), int(s[1]), int(s[2])
        p["d_u"] = line("D")
        assert len(p["d_u"]) == (p["n_free"] + 1 if p["n_free"] else 0)
        g = line("G")
        p["cg"], p["fg"] = g[0], g[1:]
        assert len(p["fg"]) == q
        if p["natural"]:
            x = line("X")
            p["shrink"] = dict(f=x[0], cg=x[1], fg=x[2:])
    return ps


def generate(ref):
    from tests import auc_ref
    ms = matrices()
    mats = [auc_ref.materialise(m) for m in ms]
    ps = problems(mats)
    for p in ps:  # every natural fold tests both classes
        y = mats[p["k"]][1]
        if p["natural"]:
            assert {float(y[t]) > 0 for t in p["test"]} == {True, False}, p["name"]
    with tempfile.TemporaryDirectory() as d:
        run_harness(build_harness(ref, d), d, mats, ps)
    rel = lambda a, b: abs(float.fromhex(a) - float.fromhex(b)) / max(abs(float.fromhex(a)), 1e-300)
    for p in ps:
        msg = f"{p['name']:28s} n_free={p['n_free']:4d} n_bound={p['n_bound']:4d} products={p['cg_iterations']:4d}"
        if p["natural"]:
            s = p["shrink"]
            msg += (f"  shrinking differs: f {rel(p['f'], s['f']):.1e} cg {rel(p['cg'], s['cg']):.1e} fg " +
                    " ".join(f"{rel(a, b):.1e}" for a, b in zip(p["fg"], s["fg"])))
        print(msg, file=sys.stderr)
    return dict(matrices=ms, problems=ps)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "auc_gradient.json")
    with open(out, "w") as f:
        json.dump(generate(sys.argv[1]), f, separators=(",", ":"))
        f.write("\n")
    print(out)
