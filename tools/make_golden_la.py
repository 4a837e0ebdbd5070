#!/usr/bin/env python3
"""Generate tests/golden/la_protein.json from the reference's own la_kernel code.

The examples and parameter sets are made here (deterministic); the values come
from tests/cpp/la_ref_harness.cpp, which this script compiles together with
the reference's bpla_kernel/{bpla_kernel,data}.cpp and
common/{rna,profile,aaprofile}.cpp, in place, into a temporary directory.
Nothing compiled from the reference is kept.

    python tools/make_golden_la.py /path/to/reference [out.json]

Values are C99 hex floats: K(x, y) for every ordered pair of examples, in exp
and SW mode, under each parameter set (values[set][mode][x * n + y]).
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AA = "ARNDCQEGHILKMFPSTWYVBZX"
SINGLE_LENGTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200]
SEED = 0x1A5EED5


def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return state, z ^ (z >> 31)


def random_protein(state, length):
    """`length` letters drawn uniformly from the 20 standard residues."""
    out = []
    for _ in range(length):
        state, r = splitmix64(state)
        out.append(AA[r % 20])
    return state, "".join(out)


def examples():
    st = SEED
    ex = []
    for n in SINGLE_LENGTHS:
        st, s = random_protein(st, n)
        ex.append([s])
    # B, Z, X, U, *, - and lowercase letters
    ex.append(["mkvBZXlaU*-wyhqBzxu-ACDEFGHIKLMNPQRSTVWY*"])
    # alignments (about 70 columns): gap columns, one column that is all '-'
    st, a = random_protein(st, 70)
    st, b = random_protein(st, 70)
    st, c = random_protein(st, 70)

    def gaps(s, at):
        s = list(s)
        for k in at:
            s[k] = "-"
        return "".join(s)

    ex.append([gaps(a, [5, 6, 7, 30, 50]), gaps(b, [12, 30, 31, 66])])
    ex.append([gaps(a, [0, 41, 69]), gaps(b[::-1], [20, 41, 42, 43]), gaps(c, [41, 55, 56])])
    # three identical rows: the single sequence of length 65
    ex.append([ex[SINGLE_LENGTHS.index(65)][0]] * 3)
    return ex


def blosum62():
    sys.path.insert(0, ROOT)
    import stem_kernel_amd as ska
    return [float(v) for v in ska.LAKernel().params.aa_score_table]


def parameter_sets():
    import numpy as np
    f32 = lambda v: float(np.float32(v))
    b62 = blosum62()
    # a non-integer, asymmetric table
    odd = [0.5 * b62[a * 23 + b] + 0.173 * ((7 * a + 3 * b) % 11 - 5) for a in range(23) for b in range(23)]
    return [dict(gap=f32(-10.0), ext=f32(-1.0), beta=f32(0.11), table=b62),
            dict(gap=-6.5, ext=-0.5, beta=0.25, table=odd)]


def build_harness(ref, workdir):
    """Compile the harness and the reference's sources into workdir."""
    exe = os.path.join(workdir, "la_ref_harness")
    shim = os.path.join(ROOT, "oracle", "ref_shim")
    src = [os.path.join(ROOT, "tests", "cpp", "la_ref_harness.cpp")]
    src += [os.path.join(ref, "bpla_kernel", f) for f in ("bpla_kernel.cpp", "data.cpp")]
    src += [os.path.join(ref, "common", f) for f in ("rna.cpp", "profile.cpp", "aaprofile.cpp")]
    subprocess.run(["g++", "-O2", "-std=gnu++11", "-ffp-contract=off", "-w", "-include", "algorithm",
                    "-I", os.path.join(shim, "standin"), "-I", shim, "-I", os.path.join(ref, "bpla_kernel"),
                    *src, "-o", exe], check=True, cwd=workdir)
    return exe


def reference_values(exe, workdir, ex, params):
    """values[set][mode][x * n + y] as hex-float strings."""
    path = os.path.join(workdir, "la_input.txt")
    with open(path, "w") as f:
        f.write(f"{len(ex)}\n")
        for rows in ex:
            f.write(f"{len(rows)}\n" + "".join(r + "\n" for r in rows))
        f.write(f"{len(params)}\n")
        for p in params:
            f.write(" ".join(float(p[k]).hex() for k in ("gap", "ext", "beta")) + "\n")
            f.write(" ".join(float(t).hex() for t in p["table"]) + "\n")
    out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split()
    n2 = len(ex) ** 2
    assert len(out) == 2 * n2 * len(params), len(out)
    return [[out[(2 * s + m) * n2:(2 * s + m + 1) * n2] for m in range(2)] for s in range(len(params))]


def generate(ref):
    ex, params = examples(), parameter_sets()
    with tempfile.TemporaryDirectory() as d:
        vals = reference_values(build_harness(ref, d), d, ex, params)
    return dict(examples=ex,
                params=[dict(gap=p["gap"].hex(), ext=p["ext"].hex(), beta=p["beta"].hex(),
                             table=[float(t).hex() for t in p["table"]]) for p in params],
                values=vals)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "la_protein.json")
    with open(out, "w") as f:
        json.dump(generate(sys.argv[1]), f, indent=0)
        f.write("\n")
    print(out)
