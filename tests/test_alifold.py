"""Consensus (alifold-style) fold of alignments: sk_fold_alignment
(csrc/kernels/fold_ali.hip), sk_dataset_add_consensus, sk_dataset_add_alifolded,
the CLI's --consensus-fold.

ViennaRNA's pf_alifold is not available: the model is DESIGN.md §9's, restated
in tests/alifold_ref.py.  Pinned here:
* the restatement's exhaustive enumerator equals the oracle's enumeration on
  single rows, and S identical rows equal one;
* the restatement's DP equals its enumerator on short alignments;
* the GPU consensus fold equals the plain GPU fold on identical gap-free rows,
  the enumerator on the hand-made alignments and the DP on longer ones
  (test_fold.py's tolerances: probabilities 1e-9 absolute, ln Z 1e-12 relative);
* an example built from a consensus matrix holds that matrix itself.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import alifold_ref as ar
from tests.helpers import fold_paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "stem_kernel_amd", "bin", "stem_kernel_lite")

ALNS = {
    "comp": ["GGGACAAAAGUCCC", "GGCACAAAAGUGCC", "GAGACAAAAGUCUC", "GGGUCAAAAGACCC"],
    "gaps": ["GGGAC-AAAGUCCC", "GGCACAAAAGUGCC", "GG-ACAAAAGU-CC"],
    "minor": ["GGGACAAAAGUCCC", "GGGACAAAAGUCCA", "GGAACAAAAGUCCC", "GGGACAAAAGUCCC", "GCGACAAAAGUCGC"],
    "multi": ["GGCGAAAGCAGCAAAGCC", "GGCGAAAGCAGCAAAGCC", "GACGAAAGCAGCAAAGUC"],
}
N_STRUCT = {"comp": 155, "gaps": 85, "minor": 155, "multi": 225}


def _rand_seq(rng, L):
    return "".join(rng.choice(list("ACGU"), L))


def _design(rng, n):
    """A stem-loop design over n columns: nested and adjacent helices of 3..6 pairs."""
    seq = list(_rand_seq(rng, n))
    pairs = []

    def fill(lo, hi):  # columns lo..hi-1
        while hi - lo >= 12:
            k = int(rng.integers(3, min(6, (hi - lo - 4) // 2) + 1))
            span = int(rng.integers(2 * k + 4, min(hi - lo, 2 * k + 24) + 1))
            i, j = lo, lo + span - 1
            for a in range(k):
                x = "GCGCAU"[int(rng.integers(0, 6))]
                y = {"G": "C", "C": "G", "A": "U", "U": "A"}[x]
                seq[i + a], seq[j - a] = x, y
                pairs.append((i + a, j - a))
            fill(i + k + 1, j - k)
            lo = j + 1 + int(rng.integers(0, 3))

    fill(int(rng.integers(0, 3)), n)
    return "".join(seq), pairs


def _mutated_alignment(rng, n, S):
    """S rows from one design: compensatory changes of its pairs, single
    changes, point mutations and gaps."""
    seq, pairs = _design(rng, n)
    canon = ["GC", "CG", "AU", "UA", "GU", "UG"]
    rows = []
    for _ in range(S):
        r = list(seq)
        for i, j in pairs:
            u = rng.random()
            if u < 0.35:
                r[i], r[j] = canon[int(rng.integers(0, 6))]
            elif u < 0.42:
                r[i] = "ACGU"[int(rng.integers(0, 4))]
        for k in range(n):
            u = rng.random()
            if u < 0.05:
                r[k] = "ACGU"[int(rng.integers(0, 4))]
            elif u < 0.09:
                r[k] = "-"
        rows.append("".join(r))
    return rows


@functools.lru_cache(maxsize=None)
def _dp(rows, no_gu=False, no_lp=False):
    """the DP restatement, computed once per alignment and shared"""
    lz, p = ar.fold_alignment_dp(list(rows), no_gu, no_lp)
    p.setflags(write=False)
    return lz, p


@functools.lru_cache(maxsize=None)
def _enum(rows, no_gu=False, no_lp=False):
    lz, p, cnt, M = ar.enumerate_alignment(list(rows), no_gu, no_lp)
    p.setflags(write=False)
    return lz, p, cnt, M


def _close(z, p, ref_z, ref_p):
    assert abs(z - ref_z) <= 1e-12 * max(1.0, abs(ref_z)), (z, ref_z)
    assert p.shape == ref_p.shape
    assert np.max(np.abs(p - ref_p), initial=0.0) < 1e-9


# ------------------------------------------------------------------ CPU: the restatements
@pytest.mark.parametrize("n", [5, 9, 12, 16])
@pytest.mark.parametrize("flags", [(0, 0), (1, 0), (0, 1)])
def test_enumerator_equals_oracle_on_single_rows(n, flags):
    rng = np.random.default_rng(1000 + n)
    for _ in range(3):
        s = _rand_seq(rng, n)
        lz, p, cnt, _ = ar.enumerate_alignment([s], bool(flags[0]), bool(flags[1]))
        b, pb, c2 = po.fold_enum(s, flags[0], 0, no_lp=bool(flags[1]))
        assert cnt == c2
        assert abs(lz - b) <= 1e-12 * max(1.0, abs(b)) and np.max(np.abs(p - pb), initial=0.0) < 1e-12, s
        lz3, p3, c3, _ = ar.enumerate_alignment([s] * 3, bool(flags[0]), bool(flags[1]))
        assert c3 == cnt
        assert abs(lz3 - lz) <= 1e-12 * max(1.0, abs(lz)) and np.max(np.abs(p3 - p), initial=0.0) < 1e-12, s


def test_named_alignments_structures_and_pscores():
    seen = set()
    for name, rows in ALNS.items():
        _, _, cnt, M = _enum(tuple(rows))
        assert cnt == N_STRUCT[name], name
        seen |= set(int(v) for v in M.pscore[M.allowed])
    assert {-200, -50, 41, 66, 75, 80, 133} <= seen


@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True)])
def test_dp_equals_enumerator(flags):
    rng = np.random.default_rng(77 + flags[0] + 2 * flags[1])
    alns = list(ALNS.values())
    alns += [_mutated_alignment(rng, n, S) for n, S in ((12, 2), (15, 3), (17, 4), (18, 3), (18, 6))]
    n_struct = 0
    for rows in alns:
        lz, p, cnt, _ = _enum(tuple(rows), *flags)
        lz2, p2 = _dp(tuple(rows), *flags)
        n_struct += cnt
        assert abs(lz - lz2) <= 1e-12 * max(1.0, abs(lz)), rows
        assert np.max(np.abs(p - p2), initial=0.0) < 1e-12, rows
    assert n_struct > 600


# ------------------------------------------------------------------ CPU: examples from a consensus matrix
def _some_matrix(rng, L, density=0.08):
    P = np.zeros(L * (L - 1) // 2)
    k = rng.choice(P.size, max(1, int(density * P.size)), replace=False)
    P[k] = rng.random(k.size) * 0.6
    return P


def test_add_consensus_one_row_equals_add():
    rng = np.random.default_rng(5)
    s = _rand_seq(rng, 40)
    P = _some_matrix(rng, 40)
    a, b = ska.Dataset(), ska.Dataset()
    a.add("+1", [s], consensus_bpp=P)
    b.add("+1", [s], bpp_rows=[P])
    assert bytes(a.export()) == bytes(b.export())


def test_add_consensus_gap_free_rows_equal_add_of_copies():
    """Four rows: the average of four copies of P is P to the last bit
    (P + P + P + P and the division by 4 are exact)."""
    rng = np.random.default_rng(6)
    rows = [_rand_seq(rng, 30) for _ in range(4)]
    P = _some_matrix(rng, 30)
    a, b = ska.Dataset(), ska.Dataset()
    a.add("-1", rows, consensus_bpp=P)
    b.add("-1", rows, bpp_rows=[P] * 4)
    assert bytes(a.export()) == bytes(b.export())


def test_add_consensus_keeps_the_matrix_under_gaps():
    """Columns 1 and 8 pair with P = 0.012 >= th = 0.01; row 2 is blank at
    column 1.  The gap-mapped average of per-row matrices holds 2/3 of it
    (below th: no node); the consensus example holds P itself: the node is
    there, and the two rows that have both letters each give P / 3."""
    rows = ["GGGAAAAACC", "GCGAAAAAGC", "G-GAAAAAUC"]
    L, i, j, pv = 10, 1, 8, 0.012
    P = np.zeros(L * (L - 1) // 2)
    P[ar.tri(L, i, j)] = pv
    ds = ska.Dataset()
    ds.add("+1", rows, consensus_bpp=P, th=0.01)
    d = ds.dag(0)
    node = [k for k in range(d["first"].size) if (d["first"][k], d["last"][k]) == (i, j)]
    assert len(node) == 1
    k = node[0]
    o = int(d["n_bpfreq"][:k].sum())
    got = d["bp_p"][o:o + int(d["n_bpfreq"][k])]
    assert got.size == 2  # rows 0 and 1: G.C and C.G
    assert np.allclose(got, np.float32(pv) / np.float32(3.0), rtol=1e-6, atol=0.0)
    # the same values as per-row matrices, gap-mapped and averaged: below th
    per_row = []
    for r in rows:
        m = [c for c in range(L) if r[c] != "-"]
        q = np.zeros(len(m) * (len(m) - 1) // 2)
        if i in m and j in m:
            q[ar.tri(len(m), m.index(i), m.index(j))] = pv
        per_row.append(q)
    av = ska.Dataset()
    av.add("+1", rows, bpp_rows=per_row, th=0.01)
    da = av.dag(0)
    assert not any((a, b) == (i, j) for a, b in zip(da["first"], da["last"]))


def test_add_consensus_errors():
    ds = ska.Dataset()
    with pytest.raises(ValueError, match="consensus_bpp"):
        ds.add("+1", ["GGGAAACCC", "GGGAAACCC"], consensus_bpp=np.zeros(9 * 8 // 2 - 1))
    with pytest.raises(ska.StemKernelError) as e:
        ds.add("+1", ["GGGAAACCC", "GGGAAACC"], consensus_bpp=np.zeros(9 * 8 // 2))
    assert e.value.code == -1
    assert len(ds) == 0


def _run_cli(args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_usage_lists_consensus_fold():
    r = _run_cli([])
    assert r.returncode == 1
    assert "--consensus-fold" in r.stdout and "--use-alifold" in r.stdout


def _consensus_method_lines(tmp_path):
    libdir = os.path.join(ROOT, "stem_kernel_amd")
    exe = str(tmp_path / "consensus_method")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "consensus_method.cpp"), "-L", libdir, "-lstem_kernel_amd",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True, timeout=300).stdout.splitlines()


CONSENSUS_LINES = ["consensus: 1 matrices, first of 66, consensus 1", "sampling: 2 matrices, first of 55, consensus 0"]


def test_compat_header_consensus_option(tmp_path):
    """BPMatrixOptions::consensus passes the method check and leaves one
    matrix over the 12 columns (it may fail later for lack of a GPU);
    n_samples > 0 wins over it; alifold still stops at the check."""
    out = _consensus_method_lines(tmp_path)
    assert len(out) == 3, out
    assert "only the FOLD" not in out[0] and "only the FOLD" not in out[1], out
    assert out[0] == CONSENSUS_LINES[0] or out[0].startswith("consensus: error: "), out[0]
    assert out[1] == CONSENSUS_LINES[1] or out[1].startswith("sampling: error: "), out[1]
    assert out[2].startswith("alifold: error: only the FOLD"), out[2]


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("flags", [{}, {"no_gu": True}, {"no_lonely_pairs": True}])
def test_gpu_identical_rows_equal_the_fold(gpu_ctx, monkeypatch, capfd, flags):
    """One row, and three identical rows, are the single-sequence fold: the
    LDS-ring path (n <= 248) and the path without it (249).  The path is the
    launch's, chosen by its longest item, so the 249-mer goes in calls of its
    own; which kernel ran is read from the driver's batch lines."""
    rng = np.random.default_rng(31)
    seqs = [_rand_seq(rng, n) for n in (5, 36, 248, 249)]
    ref, ref_z, got, lz = [], [], [], []
    for part, path in ((seqs[:3], "ring"), (seqs[3:], "hbm")):
        (r, rz), b_fold = fold_paths(capfd, monkeypatch, lambda: gpu_ctx.fold(part, log_z=True, **flags))
        (g, gz), b_ali = fold_paths(capfd, monkeypatch, lambda: gpu_ctx.fold_alignment(
            [[s] for s in part] + [[s] * 3 for s in part], with_log_z=True, **flags))
        assert b_fold == [(len(part), len(part[-1]), path)] and b_ali == [(2 * len(part), len(part[-1]), path)]
        ref += list(r) + list(r)
        ref_z += list(rz) + list(rz)
        got += list(g)
        lz += list(gz)
    assert len(got) == 2 * len(seqs)
    assert any(np.max(p, initial=0.0) > 0.1 for p in ref)
    for k in range(len(got)):
        _close(lz[k], got[k], ref_z[k], ref[k])


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True)])
def test_gpu_named_alignments_equal_enumeration(gpu_ctx, flags):
    names = list(ALNS)
    got, lz = gpu_ctx.fold_alignment([ALNS[k] for k in names], no_gu=flags[0], no_lonely_pairs=flags[1],
                                     with_log_z=True)
    for k, name in enumerate(names):
        ref_z, ref_p, _, _ = _enum(tuple(ALNS[name]), *flags)
        _close(lz[k], got[k], ref_z, ref_p)
    if flags == (False, False):
        # covariation counts: the consensus of `minor` is not the fold of its first row
        first = gpu_ctx.fold([ALNS["minor"][0]])[0]
        assert np.max(np.abs(got[names.index("minor")] - first)) > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("n,S", [(40, 4), (70, 7)])
def test_gpu_mutated_alignments_equal_dp(gpu_ctx, n, S):
    rng = np.random.default_rng(900 + n)
    rows = _mutated_alignment(rng, n, S)
    assert any("-" in r for r in rows) and len(set(rows)) == S
    for flags in ((False, False), (True, False), (False, True)):
        got, lz = gpu_ctx.fold_alignment([rows], no_gu=flags[0], no_lonely_pairs=flags[1], with_log_z=True)
        ref_z, ref_p = _dp(tuple(rows), *flags)
        assert np.max(ref_p) > 0.1
        _close(lz[0], got[0], ref_z, ref_p)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True)])
def test_gpu_longest_ring_alignment_equals_dp(gpu_ctx, monkeypatch, capfd, flags):
    """248 columns x 3 rows alone: the longest alignment the LDS-ring kernel
    takes (the 249-column, no-ring case is in test_gpu_mixed_call_keeps_order)."""
    rows = _mutated_alignment(np.random.default_rng(248003), 248, 3)
    assert any("-" in r for r in rows) and len(set(rows)) == 3
    (got, lz), batches = fold_paths(capfd, monkeypatch, lambda: gpu_ctx.fold_alignment(
        [rows], no_gu=flags[0], no_lonely_pairs=flags[1], with_log_z=True))
    assert batches == [(1, 248, "ring")]
    ref_z, ref_p = _dp(tuple(rows), *flags)
    assert np.max(ref_p) > 0.1
    _close(lz[0], got[0], ref_z, ref_p)


@pytest.mark.gpu
def test_gpu_mixed_call_keeps_order(gpu_ctx):
    """Row counts 1, 3, 7 and lengths 12, 40, 249 in one call: every output at
    its place in call order, equal to the DP and to the alignment folded alone."""
    rng = np.random.default_rng(4242)
    alns = [_mutated_alignment(rng, n, S) for n, S in ((40, 3), (12, 7), (249, 1), (12, 1), (249, 3), (40, 7))]
    got, lz = gpu_ctx.fold_alignment(alns, with_log_z=True)
    assert [p.size for p in got] == [len(a[0]) * (len(a[0]) - 1) // 2 for a in alns]
    for k, rows in enumerate(alns):
        ref_z, ref_p = _dp(tuple(rows))
        _close(lz[k], got[k], ref_z, ref_p)
    alone, lz1 = gpu_ctx.fold_alignment([alns[4]], with_log_z=True)
    assert np.array_equal(alone[0], got[4]) and lz1[0] == lz[4]


@pytest.mark.gpu
def test_gpu_64_rows_of_400_columns(gpu_ctx):
    """The documented floor of the limits: 64 rows of 400 columns run (no LDS
    ring, the tables by diagonal in HBM); identical rows, so the fold of the
    row is the reference."""
    s = _rand_seq(np.random.default_rng(64400), 400)
    ref, ref_z = gpu_ctx.fold([s], log_z=True)
    got, lz = gpu_ctx.fold_alignment([[s] * 64], with_log_z=True)
    _close(lz[0], got[0], ref_z[0], ref[0])


@pytest.mark.gpu
def test_gpu_compat_header_consensus_option(gpu_ctx, tmp_path):
    assert _consensus_method_lines(tmp_path)[:2] == CONSENSUS_LINES


@pytest.mark.gpu
def test_gpu_argument_errors(gpu_ctx):
    L = ska.lib()
    out, lz = np.zeros(64), np.zeros(2)
    f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731

    def call(rows, n_rows, flags):
        rarr = (C.c_char_p * len(rows))(*[r.encode() for r in rows])
        nr = (C.c_int32 * len(n_rows))(*n_rows)
        return L.sk_fold_alignment(gpu_ctx.handle, len(n_rows), nr, rarr, flags, f64(out), f64(lz))

    assert call(["GGGAAACCC"], [1], 0) == 0
    assert call(["GGGAAACCC"], [1], 2) == -6            # --noClosingGU: SK_ERR_UNSUPPORTED
    assert "noClosingGU" in L.sk_last_error(gpu_ctx.handle).decode()
    assert call(["GGGAAACCC", "GGGAAACC"], [2], 0) == -1  # unequal rows: SK_ERR_INVALID
    assert call(["GGGAAACCC"], [0], 0) == -1              # no rows
    with pytest.raises(ska.StemKernelError) as e:
        gpu_ctx.fold_alignment([["GGGAAACCC", "GGGAAACC"]])
    assert e.value.code == -1


def _parse_libsvm(text):
    return np.array([[float(t.split(":")[1]) for t in line.split()[2:]] for line in text.splitlines()])


@pytest.mark.gpu
def test_gpu_consensus_dataset_and_cli(gpu_ctx, tmp_path):
    """Dataset.folded(consensus=True) = examples added from fold_alignment's
    matrices = the CLI's --consensus-fold on the same CLUSTAL files (its
    libsvm text holds 6 significant digits)."""
    rng = np.random.default_rng(606)
    alns = [_mutated_alignment(rng, 36, 3) for _ in range(4)]
    ds = ska.Dataset.folded(gpu_ctx, alns, consensus=True)
    mats = gpu_ctx.fold_alignment(alns)
    ref = ska.Dataset()
    for rows, P in zip(alns, mats):
        ref.add("+1", rows, consensus_bpp=P)
    kern = ska.SuStemKernel()
    g, gr = gpu_ctx.gram(ds, kern), gpu_ctx.gram(ref, kern)
    assert g.shape == (4, 4) and np.max(np.abs(g - gr) / np.abs(gr)) <= 1e-12
    # n_samples > 0 wins over consensus (the reference's Options::method())
    smp = ska.Dataset.folded(gpu_ctx, alns, consensus=True, n_samples=50, seed=1)
    assert bytes(smp.export()) == bytes(ska.Dataset.folded(gpu_ctx, alns, n_samples=50, seed=1).export())
    for k, rows in enumerate(alns):
        with open(tmp_path / f"a{k}.aln", "w") as fh:
            fh.write("CLUSTAL W (1.83) multiple sequence alignment\n\n")
            for r, row in enumerate(rows):
                fh.write(f"seq{r}      {row}\n")
            fh.write("\n")
    args = ["--no-string", "--consensus-fold", tmp_path / "c.txt"]
    for k in range(4):
        args += ["+1", tmp_path / f"a{k}.aln"]
    r = _run_cli(args)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _parse_libsvm((tmp_path / "c.txt").read_text())
    g6 = np.array([[float(f"{v:.6g}") for v in row] for row in g])
    assert got.shape == (4, 4)
    assert np.max(np.abs(got - g6) / np.maximum(np.abs(g6), 1e-300)) <= 1e-12
    r = _run_cli(["--no-string", tmp_path / "p.txt"] + args[3:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert not np.array_equal(_parse_libsvm((tmp_path / "p.txt").read_text()), got)
