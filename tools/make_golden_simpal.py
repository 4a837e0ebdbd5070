#!/usr/bin/env python3
"""Generate tests/golden/simpal.json from the reference's own simpal code.

The sequences, base-pairing probabilities and parameters are made here
(deterministic); the maps and kernel values come from
tests/cpp/simpal_ref_harness.cpp, which includes the reference's
simpal/simpal.cpp in place and is compiled into a temporary directory.
Nothing compiled from the reference is kept.

    python tools/make_golden_simpal.py /path/to/reference [out.json]

Two groups of examples.  "exact": every (key, d) of a map is the sum of at
most two weights, so the float sum does not depend on the order the
reference's hash_multimap yields them in and the restatement must agree bit
for bit.  "ordered": three or more weights per entry; the largest count is
stored as n_max and bounds the disagreement.  Examples of one "set" share
their seed_length; the queries are all ordered pairs inside a set under the
tolerances -1, 0, 1 and seed_length.  Weights and values are C99 hex floats.
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0x51A9A1


def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return state, z ^ (z >> 31)


def random_rna(state, length):
    out = []
    for _ in range(length):
        state, r = splitmix64(state)
        out.append("acgu"[r % 4])
    return state, "".join(out)


def revcomp(s):
    return "".join({"a": "u", "c": "g", "g": "c", "u": "a"}[c] for c in reversed(s))


def bpp_of(seq):
    """The synthetic fold without GU pairs, rounded to 6 significant digits
    (short decimal numbers that read back to the same doubles)."""
    import stem_kernel_amd as ska
    return [float(f"{v:.6g}") for v in ska.fold(seq.lower(), no_gu=True)]


def examples():
    from tests import simpal_ref
    st = SEED
    ex = []

    def add(group, set_, seq, s=3, min_loop=3, max_dist=300):
        e = dict(group=group, set=set_, seq=seq, seed_length=s, min_loop=min_loop, max_dist=max_dist,
                 bpp=bpp_of(seq))
        n_max = simpal_ref.entries(seq, e["bpp"], s, min_loop, max_dist, with_multiplicity=True)[3]
        # the group's definition, asserted
        assert (n_max <= 2) if group == "exact" else (n_max >= 3), (seq, s, n_max)
        e["n_max"] = n_max
        ex.append(e)

    # exact, seed_length 3 (the CLI's defaults)
    for n in (3, 4, 7, 21, 60, 100):
        st, s = random_rna(st, n)
        add("exact", "s3", s)
    add("exact", "s3", "aaaaacaaacaaaaaca")  # no palindrome: nothing pairs with a, c
    add("exact", "s3", "GGGACtnAAAGUCCCtaGGAUCCnnGGAUCCuuAGUCC")  # t, n and uppercase letters
    st, s = random_rna(st, 21)
    add("exact", "s3", s, min_loop=0)
    st, s = random_rna(st, 60)
    add("exact", "s3", s, max_dist=20)  # cuts entries
    # exact, seed_length 1: short enough for at most two weights per entry
    for n, ml in ((8, 3), (10, 3), (6, 0)):
        while True:  # (and some weight that is not 0)
            st, s = random_rna(st, n)
            got = simpal_ref.entries(s, bpp_of(s), 1, ml, 300, with_multiplicity=True)
            if got[3] in (1, 2) and (got[2] > 0).any():
                break
        add("exact", "s1", s, s=1, min_loop=ml)
    add("exact", "s1", "acg", s=1, min_loop=0)
    # exact, seed_length 5: hairpins, so that there are entries
    for stem, loop, pad in ((8, 5, 6), (11, 9, 3)):
        st, a = random_rna(st, stem)
        st, l = random_rna(st, loop)
        st, p = random_rna(st, pad)
        add("exact", "s5", p + a + l + revcomp(a) + p[::-1], s=5)
    st, s = random_rna(st, 40)
    add("exact", "s5", s, s=5)
    # ordered: seed_length 2 on long random sequences, and low-complexity repeats
    for n, ml in ((120, 3), (90, 0)):
        while True:
            st, s = random_rna(st, n)
            if simpal_ref.entries(s, bpp_of(s), 2, ml, 300, with_multiplicity=True)[3] >= 3:
                break
        add("ordered", "o2", s, s=2, min_loop=ml)
    add("ordered", "o3", "gc" * 30)
    add("ordered", "o3", "augc" * 12 + "gcau" * 6)
    return ex


def queries(ex):
    q = []
    sets = []
    for e in ex:
        if e["set"] not in sets:
            sets.append(e["set"])
    for s in sets:
        idx = [k for k, e in enumerate(ex) if e["set"] == s]
        sl = ex[idx[0]]["seed_length"]
        for tol in sorted({-1, 0, 1, sl}):
            for x in idx:
                for y in idx:
                    q.append(dict(x=x, y=y, tolerance=tol))
    return q


def build_harness(ref, workdir):
    """Compile the harness (which includes the reference's simpal.cpp) into workdir."""
    exe = os.path.join(workdir, "simpal_ref_harness")
    subprocess.run(["g++", "-O2", "-std=gnu++11", "-ffp-contract=off", "-w",
                    "-I", os.path.join(ROOT, "tests", "cpp", "simpal_standin"),
                    "-I", os.path.join(ROOT, "oracle", "ref_shim", "standin"),
                    "-I", os.path.join(ref, "simpal"),
                    os.path.join(ROOT, "tests", "cpp", "simpal_ref_harness.cpp"), "-o", exe],
                   check=True, cwd=workdir)
    return exe


def reference_output(exe, workdir, ex, qs):
    """(entries per example as (keys, dist, weight hex strings), K hex strings per query)."""
    path = os.path.join(workdir, "simpal_input.txt")
    with open(path, "w") as f:
        f.write(f"{len(ex)}\n")
        for e in ex:
            f.write(f"{e['seq']} {e['seed_length']} {e['min_loop']} {e['max_dist']}\n")
            f.write(" ".join(float(v).hex() for v in e["bpp"]) + "\n")
        f.write(f"{len(qs)}\n")
        for q in qs:
            f.write(f"{q['x']} {q['y']} {q['tolerance']}\n")
    out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split("\n")
    pos, ents = 0, []
    for _ in ex:
        tag, m = out[pos].split()
        assert tag == "E"
        rows = [l.split() for l in out[pos + 1:pos + 1 + int(m)]]
        ents.append(([r[0] for r in rows], [int(r[1]) for r in rows], [r[2] for r in rows]))
        pos += 1 + int(m)
    vals = [l for l in out[pos:] if l]
    assert len(vals) == len(qs), (len(vals), len(qs))
    return ents, vals


def generate(ref):
    ex = examples()
    qs = queries(ex)
    with tempfile.TemporaryDirectory() as d:
        ents, vals = reference_output(build_harness(ref, d), d, ex, qs)
    for e, (k, dd, w) in zip(ex, ents):
        e["keys"], e["dist"], e["weight"] = k, dd, w
    for q, v in zip(qs, vals):
        q["K"] = v
    return dict(examples=ex, queries=qs)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "simpal.json")
    with open(out, "w") as f:
        json.dump(generate(sys.argv[1]), f, separators=(",", ":"))
        f.write("\n")
    print(out)
