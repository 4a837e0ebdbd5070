#!/usr/bin/env python3
"""Generate tests/golden/la_protein_grad.json from the reference's own
compute_gradients (BPLAKernel<double,AAMData>, bpla_kernel.cpp:385-401).

The examples and parameter sets are make_golden_la.py's; the numbers come
from tests/cpp/la_grad_ref_harness.cpp, which this script compiles together
with the reference's sources, in place, into a temporary directory with
make_golden_la.py's compile line.  Nothing compiled from the reference is
kept.

    python tools/make_golden_la_grad.py /path/to/reference [out.json]

Values are C99 hex floats, per parameter set and ordered pair (index
x * n + y): value, d_beta, d_gap, d_ext.  d_alpha is +0.0 for every pair
(asserted here) and is not stored.
"""
import json
import math
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_la as base  # noqa: E402

ROOT = base.ROOT
FIELDS = ("value", "d_beta", "d_gap", "d_ext")


def build_harness(ref, workdir):
    """make_golden_la.build_harness's compile line over la_grad_ref_harness.cpp."""
    exe = os.path.join(workdir, "la_grad_ref_harness")
    shim = os.path.join(ROOT, "oracle", "ref_shim")
    src = [os.path.join(ROOT, "tests", "cpp", "la_grad_ref_harness.cpp")]
    src += [os.path.join(ref, "bpla_kernel", f) for f in ("bpla_kernel.cpp", "data.cpp")]
    src += [os.path.join(ref, "common", f) for f in ("rna.cpp", "profile.cpp", "aaprofile.cpp")]
    subprocess.run(["g++", "-O2", "-std=gnu++11", "-ffp-contract=off", "-w", "-include", "algorithm",
                    "-I", os.path.join(shim, "standin"), "-I", shim, "-I", os.path.join(ref, "bpla_kernel"),
                    *src, "-o", exe], check=True, cwd=workdir)
    return exe


def write_input(path, ex, params):
    """la_ref_harness.cpp's input format."""
    with open(path, "w") as f:
        f.write(f"{len(ex)}\n")
        for rows in ex:
            f.write(f"{len(rows)}\n" + "".join(r + "\n" for r in rows))
        f.write(f"{len(params)}\n")
        for p in params:
            f.write(" ".join(float(p[k]).hex() for k in ("gap", "ext", "beta")) + "\n")
            f.write(" ".join(float(t).hex() for t in p["table"]) + "\n")


def reference_values(exe, workdir, ex, params):
    """values[set] = dict(value, d_beta, d_gap, d_ext), each a list of n * n
    hex-float strings; checks what the fixture's users rely on."""
    path = os.path.join(workdir, "la_grad_input.txt")
    write_input(path, ex, params)
    lines = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines()
    n2 = len(ex) ** 2
    assert len(lines) == n2 * len(params), len(lines)
    out = []
    for s in range(len(params)):
        cols = {k: [] for k in FIELDS}
        for line in lines[s * n2:(s + 1) * n2]:
            v, da, db, dg, de = line.split()
            nums = [float.fromhex(t) for t in (v, da, db, dg, de)]
            assert all(math.isfinite(t) for t in nums), line
            assert nums[1] == 0.0 and math.copysign(1.0, nums[1]) == 1.0, line  # d_alpha is +0.0
            # no component is nearly cancelled: an elementwise relative comparison is meaningful
            assert all(t == 0.0 or abs(t) >= 1e-3 * abs(nums[0]) for t in nums[2:]), line
            for k, t in zip(FIELDS, (v, db, dg, de)):
                cols[k].append(t)
        out.append(cols)
    return out


def generate(ref):
    ex, params = base.examples(), base.parameter_sets()
    with tempfile.TemporaryDirectory() as d:
        vals = reference_values(build_harness(ref, d), d, ex, params)
    return dict(examples=ex,
                params=[dict(gap=p["gap"].hex(), ext=p["ext"].hex(), beta=p["beta"].hex(),
                             table=[float(t).hex() for t in p["table"]]) for p in params],
                values=vals)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "la_protein_grad.json")
    with open(out, "w") as f:
        json.dump(generate(sys.argv[1]), f, indent=0)
        f.write("\n")
    print(out)
