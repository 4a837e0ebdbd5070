#!/usr/bin/env python3
"""Generate tests/golden/svm_formulations.json from the reference's own
solve_nu_svc, solve_one_class, solve_epsilon_svr and solve_nu_svr, run with
shrinking = 0.

The Grams are the ones of tools/make_golden_svm_train.py (three integer Grams
stored as their seeds, one RBF Gram stored as hex floats); the SVR targets are
multiples of 1/4 in [-8, 8] from a splitmix64 stream per Gram.  Coefficients
(what svm_train_one leaves in alpha), rho, obj, r, the iteration count and
the solver's counts of positions at the upper bound and strictly inside come
from tests/cpp/svm_formulations_ref_harness.cpp, which includes the
reference's libsvm/svm.cpp, solver.cpp and qmatrix.cpp in place and is
compiled into a temporary directory.  Nothing compiled from the reference is
kept.

    python tools/make_golden_svm_formulations.py /path/to/reference [out.json]

Every uncapped record must converge in under 40,000 iterations (asserted).
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
NO_CAP = 10_000_000
TYPES = {"nu_svc": 1, "one_class": 2, "epsilon_svr": 3, "nu_svr": 4}
TARGET_SEED = 0x5A17D000


def targets(gram_index, n):
    """n multiples of 1/4 in [-8, 8]."""
    from tests import svm_ref
    r = svm_ref.splitmix64_stream(TARGET_SEED + gram_index, n)
    return [(int(v) % 65 - 32) / 4.0 for v in r]


def problems(labels):
    """labels[g]: the class labels of Gram g (for the nu-SVC feasibility edge)."""
    ps = []

    def add(name, ty, gram, train, C=1.0, nu=0.5, p=0.1, eps=1e-3, max_iter=NO_CAP):
        ps.append(dict(name=f"{ty}: {name}", svm_type=ty, gram=gram, train=[int(t) for t in train], C=C, nu=nu, p=p,
                       eps=eps, max_iter=max_iter))

    all300 = list(range(300))
    perm = [(k * 37 + 11) % 150 for k in range(150)]  # 37 and 150 are coprime
    two = {"nu_svc": (dict(nu=0.2), dict(nu=0.6)), "one_class": (dict(nu=0.1), dict(nu=0.5)),
           "epsilon_svr": (dict(C=0.25, p=0.5), dict(C=2.0, p=0.125)),
           "nu_svr": (dict(C=0.25, nu=0.5), dict(C=2.0, nu=0.25))}
    for ty in TYPES:
        add("l = 2", ty, 0, [0, 1])
        add("identical pair, l = 2 (TAU)", ty, 2, [0, 1])
        add("rbf l = 40", ty, 3, range(40))
        for kw in two[ty]:
            add("int300 " + " ".join(f"{k}={v:g}" for k, v in kw.items()), ty, 0, all300, **kw)
        add("indefinite", ty, 1, range(60))
        add("permuted partial list", ty, 0, perm)
        add("max_iter 7", ty, 0, all300, max_iter=7)
    # nu-SVC: nu l / 2 integer (75) and fractional (49.5); nu l / 2 == min(n+, n-) exactly
    add("nu l / 2 integer", "nu_svc", 0, all300, nu=0.5)
    add("nu l / 2 fractional", "nu_svc", 0, all300, nu=0.33)
    pos = [k for k in all300 if labels[0][k] > 0][:24]
    neg = [k for k in all300 if labels[0][k] <= 0][:40]
    add("nu l / 2 == min(n+, n-)", "nu_svc", 0, sorted(pos + neg), nu=0.75)  # 0.75 * 64 / 2 = 24
    # one-class: (int)(nu l) == l, and a fractional remainder (0.37 * 40 = 14.8)
    add("nu = 1", "one_class", 3, range(40), nu=1.0)
    add("fractional nu l", "one_class", 3, range(40), nu=0.37)
    # nu-SVR: C nu l / 2 = 37.5 runs out at example 18 of 300
    add("start point runs out", "nu_svr", 0, all300, C=2.0, nu=0.125)
    # epsilon-SVR: p = 0, and p over every |target| (all coefficients zero)
    add("p = 0", "epsilon_svr", 3, range(40), p=0.0)
    add("p over every |target|", "epsilon_svr", 0, all300, p=9.0)
    return ps


def build_harness(ref, workdir):
    """Compile the harness (which includes the reference's solver) into workdir."""
    exe = os.path.join(workdir, "svm_formulations_ref_harness")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-w", "-I", ref, "-I", os.path.join(ref, "libsvm"),
                    os.path.join(ROOT, "tests", "cpp", "svm_formulations_ref_harness.cpp"), "-o", exe],
                   check=True, cwd=workdir)
    return exe


def run_harness(exe, workdir, mats, ps):
    """mats[g] = (K, labels, targets)."""
    path = os.path.join(workdir, "svm_input.txt")
    with open(path, "w") as f:
        f.write(f"{len(mats)}\n")
        for K, y, tg in mats:
            f.write(f"{len(y)}\n" + " ".join(str(int(v)) for v in y) + "\n" +
                    " ".join(float(v).hex() for v in tg) + "\n" +
                    " ".join(float(v).hex() for v in K.reshape(-1)) + "\n")
        f.write(f"{len(ps)}\n")
        for p in ps:
            f.write(f"{p['gram']} {TYPES[p['svm_type']]} {len(p['train'])} {float(p['C']).hex()} "
                    f"{float(p['nu']).hex()} {float(p['p']).hex()} {float(p['eps']).hex()} {p['max_iter']}\n" +
                    " ".join(map(str, p["train"])) + "\n")
    out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split("\n")
    res = []
    for k, p in enumerate(ps):
        tag, iters, capped, n_bound, n_free = out[3 * k].split()
        assert tag == "P"
        coef = out[3 * k + 1].split()
        rho, obj, r = out[3 * k + 2].split()
        assert len(coef) == len(p["train"])
        res.append(dict(iterations=int(iters), status=int(capped), n_bound=int(n_bound), n_free=int(n_free),
                        coef=coef, rho=rho, obj=obj, r=r))
    return res


def generate(ref):
    import numpy as np
    import make_golden_svm_train as base
    from tests import svm_ref
    grams = [dict(g) for g in base.INT_GRAMS] + [base.rbf_gram()]
    mats = []
    for gi, g in enumerate(grams):
        if g["kind"] == "int":
            K, y = svm_ref.int_gram(g["seed"], g["n"], g["d"], g["shift"], g["indef"], g["dup"])
            g["labels"] = [int(v) for v in y]
        else:
            K = np.array([float.fromhex(v) for v in g["values"]]).reshape(g["n"], g["n"])
            y = np.array(g["labels"], dtype=np.float64)
        g["targets"] = targets(gi, g["n"])
        mats.append((K, y, g["targets"]))
    ps = problems([m[1] for m in mats])
    with tempfile.TemporaryDirectory() as d:
        res = run_harness(build_harness(ref, d), d, mats, ps)
    for p, r in zip(ps, res):
        assert r["status"] == (1 if p["max_iter"] != NO_CAP else 0), (p["name"], r["iterations"])
        assert r["iterations"] < 40_000, (p["name"], r["iterations"])
        p.update(r)
        print(f"{p['name']:48s} l={len(p['train']):4d} iter={p['iterations']:6d} n_bound={p['n_bound']:4d} "
              f"n_free={p['n_free']:4d} r={float.fromhex(p['r']):.4g}", file=sys.stderr)
    by_name = {p["name"]: p for p in ps}
    assert all(float.fromhex(c) == 0.0 for c in by_name["epsilon_svr: p over every |target|"]["coef"])
    assert all(float.fromhex(c) == 1.0 for c in by_name["one_class: nu = 1"]["coef"])
    return dict(grams=grams, problems=ps)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "svm_formulations.json")
    with open(out, "w") as f:
        json.dump(generate(sys.argv[1]), f, separators=(",", ":"))
        f.write("\n")
    print(out)
