#!/usr/bin/env python3
"""Generate tests/golden/svm_train_shrink.json from the reference's own SMO
solver run with shrinking = 1.

The Grams are the ones of tools/make_golden_svm_train.py (three integer Grams
stored as their seeds, one RBF Gram stored as hex floats); alphas, rho, obj,
the iteration count, the status and the seven counters of sk_svm_shrink_info
come from tests/cpp/svm_shrink_ref_harness.cpp, which includes the reference's
libsvm/solver.cpp and libsvm/qmatrix.cpp in place and is compiled into a
temporary directory.  Nothing compiled from the reference is kept.

    python tools/make_golden_svm_shrink.py /path/to/reference [out.json]

What the fixture as a whole must contain is asserted below (COVERAGE): if a
condition fails, add a problem.  Problems whose run never reaches a shrink
call must equal the record without shrinking (tests/golden/svm_train.json).
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
INFO = ("shrink_calls", "shrunk_calls", "min_active", "unshrunk", "regrown", "reconstructions", "resumed")


def problems():
    from tests import svm_ref
    ps = []

    def add(name, gram, train, Cp=1.0, Cn=None, eps=1e-3, max_iter=NO_CAP):
        ps.append(dict(name=name, gram=gram, train=[int(t) for t in train], Cp=Cp, Cn=Cp if Cn is None else Cn,
                       eps=eps, max_iter=max_iter))

    all300 = list(range(300))
    for C in (2.0 ** -3, 1.0, 2.0 ** 6):
        add(f"int300 C={C:g}", 0, all300, C)
    add("int300 Cp != Cn", 0, all300, 2.0, 0.5)
    add("partial list", 0, all300[2::3])
    add("range(64) C=64", 0, range(64), 64.0)
    add("range(65) C=8", 0, range(65), 8.0)
    add("range(257) C=4", 0, range(257), 4.0)
    for cv in range(5):
        add(f"split ncv=5 cv={cv}", 0, svm_ref.split(300, 5, cv)[0])
    add("l = 3", 0, [2, 1, 0])
    add("l = 2", 0, [0, 1])
    add("indefinite C=64", 1, range(60), 64.0)
    add("identical pair inside", 2, range(40), 4.0)
    add("rbf C=1", 3, range(40))
    add("rbf C=64", 3, range(40), 64.0)
    perm = [(k * 37 + 11) % 150 for k in range(150)]  # 37 and 150 are coprime
    add("permuted list", 0, perm)
    add("max_iter 7", 0, all300, 1.0, max_iter=7)
    add("max_iter 250, l = 100", 0, all300[2::3], 1.0, max_iter=250)
    add("max_iter 700, int300 C=1", 0, all300, 1.0, max_iter=700)
    return ps


def build_harness(ref, workdir):
    """Compile the harness (which includes the reference's solver) into workdir."""
    exe = os.path.join(workdir, "svm_shrink_ref_harness")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-w", "-I", ref, "-I", os.path.join(ref, "libsvm"),
                    os.path.join(ROOT, "tests", "cpp", "svm_shrink_ref_harness.cpp"), "-o", exe],
                   check=True, cwd=workdir)
    return exe


def run_harness(exe, workdir, grams, ps):
    from tests import svm_ref
    path = os.path.join(workdir, "svm_input.txt")
    with open(path, "w") as f:
        f.write(f"{len(grams)}\n")
        for g in grams:
            if g["kind"] == "int":
                f.write(f"I {g['seed']} {g['n']} {g['d']} {g['shift']} {g['indef']} {g['dup']}\n")
            else:
                f.write(f"S {g['n']}\n" + " ".join(str(v) for v in g["labels"]) + "\n" +
                        " ".join(g["values"]) + "\n")
        f.write(f"{len(ps)}\n")
        for p in ps:
            f.write(f"{p['gram']} {len(p['train'])} {float(p['Cp']).hex()} {float(p['Cn']).hex()} "
                    f"{float(p['eps']).hex()} {p['max_iter']}\n" + " ".join(map(str, p["train"])) + "\n")
    out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split("\n")
    pos = 0
    for g in grams:
        if g["kind"] != "int":
            continue
        tok = out[pos].split()
        pos += 1
        assert tok[0] == "G"
        K, y = svm_ref.int_gram(g["seed"], g["n"], g["d"], g["shift"], g["indef"], g["dup"])
        # the Python twin of the harness's generator makes the same Gram
        assert float.fromhex(tok[1]) == float(K.sum()) and [int(v) for v in tok[2:]] == [int(v) for v in y], g
        g["labels"] = [int(v) for v in y]
    res = []
    for p in ps:
        tok = out[pos].split()
        assert tok[0] == "P" and len(tok) == 4 + len(INFO)
        alpha = out[pos + 1].split()
        rho, obj = out[pos + 2].split()
        pos += 3
        assert len(alpha) == len(p["train"])
        res.append(dict(iterations=int(tok[1]), status=int(tok[2]), capped_active=int(tok[3]), alpha=alpha,
                        rho=rho, obj=obj, info=dict(zip(INFO, map(int, tok[4:])))))
    return res


def check_coverage(ps):
    """COVERAGE: what the fixture as a whole must contain."""
    info = [p["info"] for p in ps]
    ls = [len(p["train"]) for p in ps]
    assert sum(4 * i["min_active"] < l for i, l in zip(info, ls)) >= 5, "min_active < l/4 on five problems"
    assert sum(i["unshrunk"] for i in info) >= 3, "three problems that unshrink"
    assert sum(i["regrown"] for i in info) >= 1, "a problem whose unshrink branch grows the active set"
    assert sum(i["resumed"] > 0 for i in info) >= 2, "two problems that go on after a reconstruction"
    # capped while shrunk: capped_active is the active size at the selection the cap replaced
    by_name = {p["name"]: p for p in ps}
    for capped, whole, cap in (("max_iter 250, l = 100", "partial list", 250),
                               ("max_iter 700, int300 C=1", "int300 C=1", 700)):
        c, w = by_name[capped], by_name[whole]
        assert c["status"] == 1 and c["iterations"] == cap < w["iterations"], capped
        assert 0 < c["capped_active"] < len(c["train"]), capped
    assert by_name["max_iter 7"]["status"] == 1 and by_name["max_iter 7"]["info"]["shrink_calls"] == 0
    i = by_name["l = 3"]["info"]
    assert (i["shrink_calls"], i["shrunk_calls"], i["unshrunk"]) == (2, 0, 1), i
    # no shrink call: the run is the one without shrinking
    with open(os.path.join(ROOT, "tests", "golden", "svm_train.json")) as f:
        off = {p["name"]: p for p in json.load(f)["problems"]}
    for name in ("l = 2", "int300 C=0.125", "int300 Cp != Cn"):
        p, q = by_name[name], off[name]
        assert p["info"]["shrink_calls"] == 0 and p["info"]["min_active"] == len(p["train"]), name
        assert p["train"] == q["train"] and (p["Cp"], p["Cn"], p["eps"]) == (q["Cp"], q["Cn"], q["eps"])
        assert all(p[k] == q[k] for k in ("alpha", "rho", "obj", "iterations")), name
    # and the runs that shrink are not that run
    assert sum(p["alpha"] != off[p["name"]]["alpha"] for p in ps if p["name"] in off) >= 5


def generate(ref):
    import make_golden_svm_train as base
    grams = [dict(g) for g in base.INT_GRAMS] + [base.rbf_gram()]
    ps = problems()
    with tempfile.TemporaryDirectory() as d:
        res = run_harness(build_harness(ref, d), d, grams, ps)
    for p, r in zip(ps, res):
        assert r["status"] == (1 if p["max_iter"] != NO_CAP else 0), (p["name"], r["iterations"])
        p.update(r)
        print(f"{p['name']:32s} l={len(p['train']):4d} iter={p['iterations']:6d}  " +
              " ".join(f"{k}={v}" for k, v in p["info"].items()), file=sys.stderr)
    check_coverage(ps)
    return dict(grams=grams, problems=ps)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "svm_train_shrink.json")
    with open(out, "w") as f:
        json.dump(generate(sys.argv[1]), f, separators=(",", ":"))
        f.write("\n")
    print(out)
