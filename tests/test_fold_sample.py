"""Stochastic structure sampling (sk_fold_sample, csrc/kernels/fold_sample.hip):
BPMatrix SFOLD, common/bpmatrix.cpp:179-232 (--sampling N).

Every reference value comes from the oracle (oracle/fold_oracle.c), never
from the engine's own fold: P(structure) = exp(-E/kT - ln Z) with E from
po.fold_structure_energy and ln Z from po.fold_mccaskill; P(pair) is the
oracle's bpp.  Samples are independent, so the count of a structure or of a
pair among S samples is exactly Binomial(S, p) under a correct sampler, and
the allowed deviation is

    |c/S - p| <= 7 sqrt(p (1 - p) / S) + 4 / S

-- a condition from the binomial law, not a measurement: its tail is below
1e-9 per cell, and the seeds are fixed, so the outcome is deterministic.

The designed sequences A-E put real mass on many structures (random 14-18-mers
have ln Z ~ 0: the empty structure takes > 99 %).  B holds the multiloop
structure (((.((....)).((....)).))) at E = 240 dcal/mol, pi = 0.00735."""
import collections
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from stem_kernel_amd._lib import SIGNATURES, lib
from tests.helpers import fold_paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "stem_kernel_amd")
CLI = os.path.join(LIBDIR, "bin", "stem_kernel_lite")

KT = (37 + 273.15) * 1.98717 / 10  # dcal/mol
SEQS = {
    "A": "GGGGAAACCCC",
    "B": "GGGAGCGAAAGCAGCGAAAGCACCC",
    "C": "GGCGAAAGCCGGCGAAAGCC",
    "D": "GCGCAAGGAAACCUGCGC",
    "E": "GGUGAAAUGCC",
}
B_MULTILOOP = "(((.((....)).((....)).)))"
FLAGS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]  # no_gu, no_closing_gu, no_lonely_pairs


def _bound(p, s):
    return 7.0 * np.sqrt(p * (1.0 - p) / s) + 4.0 / s


def _kw(f):
    return dict(no_gu=bool(f[0]), no_closing_gu=bool(f[1]), no_lonely_pairs=bool(f[2]))


def _random(length):
    return ska.random_sequences(1, length, 0x5EED0700 + length)[0]


def _pairs(db):
    st, out = [], []
    for k, ch in enumerate(db):
        if ch == "(":
            st.append(k)
        elif ch == ")":
            assert st, db
            out.append((st.pop(), k))
        else:
            assert ch == ".", db
    assert not st, db
    return out


def _tri(n, i, j):
    return i * n - i * (i + 1) // 2 + (j - i - 1)


_ORACLE = {}


def _oracle(seq, f):
    """(ln Z, bpp) of the oracle, computed once per (sequence, flags)."""
    key = (seq, tuple(f))
    if key not in _ORACLE:
        _ORACLE[key] = po.fold_mccaskill(seq, bool(f[0]), bool(f[1]), bool(f[2]))
    return _ORACLE[key]


# ------------------------------------------------------------------ CPU
def test_symbols_exported_with_signatures():
    for name in ("sk_fold_sample", "sk_dataset_add_sampled", "sk_fold_sample_uniform"):
        assert name in SIGNATURES
        assert getattr(lib(), name) is not None


def test_invalid_arguments_before_any_device_work():
    L = lib()
    seqs = (C.c_char_p * 1)(b"GGGGAAACCCC")
    out = np.zeros(64)
    po_ = out.ctypes.data_as(C.POINTER(C.c_double))
    assert L.sk_fold_sample(None, 1, seqs, 0, 10, 0, po_, None, None) == -1
    assert L.sk_fold_sample(None, 1, seqs, 0, 0, 0, po_, None, None) == -1
    assert L.sk_fold_sample(None, 1, seqs, 0, 10, 0, None, None, None) == -1
    assert L.sk_dataset_add_sampled(None, None, 0, 1, None, None, C.c_float(0.01), 0, 0, 0, 1) == -1


@pytest.mark.gpu
def test_invalid_arguments_on_a_context(gpu_ctx):
    L = lib()
    seqs = (C.c_char_p * 1)(b"GGGGAAACCCC")
    out = np.zeros(64)
    po_ = out.ctypes.data_as(C.POINTER(C.c_double))
    assert L.sk_fold_sample(gpu_ctx.handle, 1, seqs, 0, 0, 0, po_, None, None) == -1
    assert L.sk_fold_sample(gpu_ctx.handle, 1, seqs, 0, -3, 0, po_, None, None) == -1
    assert L.sk_fold_sample(gpu_ctx.handle, 1, seqs, 0, 10, 0, None, None, None) == -1
    assert L.sk_fold_sample(gpu_ctx.handle, 1, seqs, 8, 10, 0, po_, None, None) == -6
    with pytest.raises(ska.StemKernelError):
        gpu_ctx.fold_sample(["GGGGAAACCCC"], 0)


def test_uniform_generator():
    u = lib().sk_fold_sample_uniform
    assert u(5, 1, 2, 3) == u(5, 1, 2, 3)
    base = u(5, 1, 2, 3)
    assert len({base, u(6, 1, 2, 3), u(5, 2, 2, 3), u(5, 1, 3, 3), u(5, 1, 2, 4)}) == 5
    n = 100000
    x = np.array([u(11, 0, 0, k) for k in range(n)])
    assert x.min() >= 0.0 and x.max() < 1.0
    assert abs(x.mean() - 0.5) <= 0.005
    h = np.bincount((x * 16).astype(int), minlength=16) / n
    sigma = math.sqrt((1 / 16) * (15 / 16) / n)
    assert np.all(np.abs(h - 1 / 16) <= 7 * sigma), h
    # the streams of neighbouring samples and sequences are unrelated too
    y = np.array([u(11, 0, k, 0) for k in range(n)])
    z = np.array([u(11, k, 0, 0) for k in range(n)])
    for v in (y, z):
        assert abs(v.mean() - 0.5) <= 0.005
        hv = np.bincount((v * 16).astype(int), minlength=16) / n
        assert np.all(np.abs(hv - 1 / 16) <= 7 * sigma), hv


def _run_cli(args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_usage_lists_sampling():
    r = _run_cli([])
    assert r.returncode == 1
    assert "--sampling arg" in r.stdout and "--sampling-seed" in r.stdout
    assert "use stochastic sampling for producing base pairing probability" in r.stdout


@pytest.mark.parametrize("opt,val", [("--sampling", "abc"), ("--sampling", "-5"), ("--sampling", "12x"),
                                     ("--sampling-seed", "abc")])
def test_cli_bad_sampling_value(tmp_path, opt, val):
    r = _run_cli([opt, val, tmp_path / "o.txt", "+1", tmp_path / "a.fa"])
    assert r.returncode == 1 and "invalid" in r.stderr and opt in r.stderr


def test_compat_header_accepts_sampling(tmp_path):
    """BPMatrixOptions with n_samples = 10 passes the method check (it may
    fail later for lack of a GPU); alifold still stops there."""
    exe = str(tmp_path / "sampling_method")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "sampling_method.cpp"), "-L", LIBDIR, "-lstem_kernel_amd",
                    f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=300).stdout.splitlines()
    assert len(out) == 2, out
    assert out[0].startswith("sampling: ") and "only the FOLD" not in out[0], out[0]
    assert out[0] == "sampling: folded 1 row" or out[0].startswith("sampling: error: "), out[0]
    assert out[1].startswith("alifold: error: only the FOLD"), out[1]


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("f", [(0, 0, 0), (1, 0, 0), (0, 1, 0)])
def test_gpu_sampled_structures_are_valid(gpu_ctx, f):
    seqs = list(SEQS.values()) + [_random(40), _random(75)]
    s = 2048
    bpp, strs = gpu_ctx.fold_sample(seqs, s, seed=1, structures=True, **_kw(f))
    for seq, p, ss in zip(seqs, bpp, strs):
        n = len(seq)
        assert len(ss) == s and all(len(x) == n for x in ss)
        cnt = np.zeros(n * (n - 1) // 2)
        for db, c in collections.Counter(ss).items():
            assert set(db) <= set("(.)")
            for i, j in _pairs(db):
                cnt[_tri(n, i, j)] += c
            assert po.fold_structure_energy(seq, db, no_gu=bool(f[0]), no_closing_gu=bool(f[1])) < 1e299, db
        assert np.array_equal(p, cnt / s)


@pytest.mark.gpu
@pytest.mark.parametrize("name,f", [("A", (0, 0, 0)), ("B", (0, 0, 0)), ("C", (0, 0, 0)), ("D", (0, 0, 0)),
                                    ("E", (0, 0, 0)), ("E", (1, 0, 0)), ("D", (0, 1, 0))])
def test_gpu_structure_distribution(gpu_ctx, name, f):
    seq = SEQS[name]
    s = 16384
    _, strs = gpu_ctx.fold_sample([seq], s, seed=2, structures=True, **_kw(f))
    lz, _ = _oracle(seq, f)
    hist = collections.Counter(strs[0])
    worst = 0.0
    for db, c in hist.items():
        e = po.fold_structure_energy(seq, db, no_gu=bool(f[0]), no_closing_gu=bool(f[1]))
        assert e < 1e299, db
        pi = math.exp(-e / KT - lz)
        dev, lim = abs(c / s - pi), _bound(pi, s)
        worst = max(worst, dev / lim)
        assert dev <= lim, (db, c, pi)
    print(f"{name} {f}: {len(hist)} distinct structures, worst deviation {worst:.3f} of the bound")
    if name == "B":
        assert B_MULTILOOP in hist
        assert po.fold_structure_energy(seq, B_MULTILOOP) == pytest.approx(240.0)


@pytest.mark.gpu
@pytest.mark.parametrize("length,s", [(40, 8192), (75, 8192), (200, 4096), (260, 4096)])
@pytest.mark.parametrize("f", FLAGS)
def test_gpu_pair_marginals(gpu_ctx, monkeypatch, capfd, length, s, f):
    """260 nucleotides: the inside launch whose tables the sampler walks runs
    without the LDS ring (more than 248), the others with it."""
    seq = _random(length)
    (bpp, lz), batches = fold_paths(capfd, monkeypatch,
                                    lambda: gpu_ctx.fold_sample([seq], s, seed=3, log_z=True, **_kw(f)))
    assert batches == [(1, length, "ring" if length <= 248 else "hbm")]
    ref_z, ref = _oracle(seq, f)
    dev = np.abs(bpp[0] - ref)
    lim = _bound(ref, s)
    print(f"L={length} {f}: worst deviation {np.max(dev / lim):.3f} of the bound, "
          f"{int(np.count_nonzero(bpp[0]))} sampled pairs")
    assert np.all(dev <= lim)
    assert abs(lz[0] - ref_z) <= 1e-12 * abs(ref_z)


@pytest.mark.gpu
def test_gpu_keying(gpu_ctx):
    seqs = [SEQS["B"], _random(75)]
    a, sa = gpu_ctx.fold_sample(seqs, 1000, seed=4, structures=True)
    b, sb = gpu_ctx.fold_sample(seqs, 1000, seed=4, structures=True)
    assert sa == sb and all(np.array_equal(x, y) for x, y in zip(a, b))
    _, sc = gpu_ctx.fold_sample(seqs, 1000, seed=5, structures=True)
    assert sc[0] != sa[0] and sc[1] != sa[1]
    # sample s is the same structure whatever the number of samples is
    _, sd = gpu_ctx.fold_sample(seqs, 100, seed=4, structures=True)
    assert sd[0] == sa[0][:100] and sd[1] == sa[1][:100]
    # the sequence index is a key: a sequence moved to another place in the call draws other samples
    _, se = gpu_ctx.fold_sample(seqs[::-1], 100, seed=4, structures=True)
    assert se[1] != sd[0]
    # a 1,200-nt sequence in the call: no LDS ring for any sequence of the launch and tables 19 KB longer,
    # still in LDS (about 21 KB), its ln Z against the oracle.  The kernel that reads the hairpin / scale
    # tables from HBM takes over from about 9,550 nt only (8 (2 L + 156) + L > 163,584 bytes), past the
    # double range: test_fold_paths.py runs it (SK_FOLD_PATH=gtab) and the sampler after it.
    long_ = _random(1200)
    short = gpu_ctx.fold_sample(seqs, 100, seed=4)
    both, lz = gpu_ctx.fold_sample(seqs + [long_], 100, seed=4, log_z=True)
    assert all(np.array_equal(x, y) for x, y in zip(short, both[:2]))
    ref_z, _ = _oracle(long_, (0, 0, 0))
    assert abs(lz[2] - ref_z) <= 1e-12 * abs(ref_z)
    assert 0.0 < both[2].max() <= 1.0


@pytest.mark.gpu
def test_gpu_edge_cases(gpu_ctx):
    seqs = ["", "A", "ACGU", "NNNNNNNNNN"]
    bpp, strs, lz = gpu_ctx.fold_sample(seqs, 64, seed=6, structures=True, log_z=True)
    for seq, p, ss in zip(seqs, bpp, strs):
        assert ss == ["." * len(seq)] * 64
        assert p.size == len(seq) * (len(seq) - 1) // 2 and not p.any()
    assert np.all(np.abs(lz) < 1e-12)


@pytest.mark.gpu
def test_gpu_dataset_path_and_fold_untouched(gpu_ctx):
    seqs = ska.random_sequences(4, 70, 0x5EED0711)
    before = gpu_ctx.fold(seqs, log_z=True)
    ds = ska.Dataset.folded(gpu_ctx, seqs, n_samples=500, seed=3)
    ref = ska.Dataset.from_sequences(seqs, bpp=gpu_ctx.fold_sample([s.lower() for s in seqs], 500, seed=3))
    assert len(ds) == len(ref) == 4
    n_pairs = 0
    for i in range(4):
        a, b = ds.dag(i), ref.dag(i)
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), (i, k)
        n_pairs += a["bp_p"].size
    assert n_pairs > 0
    # the inside_only switch leaks nothing into the next plain fold
    after = gpu_ctx.fold(seqs, log_z=True)
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0]))
    assert np.array_equal(before[1], after[1])


def _parse_libsvm(text):
    return np.array([[float(t.split(":")[1]) for t in line.split()[2:]] for line in text.splitlines()])


@pytest.mark.gpu
def test_gpu_cli_sampling(gpu_ctx, tmp_path):
    """The CLI folds each example in a call of its own (sequence index 0).
    Its libsvm text holds 6 significant digits, so the Python path's Gram is
    rounded the same way before the two are compared to 1e-12 relative."""
    seqs = ska.random_sequences(4, 70, 0x5EED0712)
    with open(tmp_path / "a.fa", "w") as fh:
        for k, s in enumerate(seqs):
            fh.write(f">s{k}\n{s}\n")
    r = _run_cli(["--no-string", "--sampling", "200", "--sampling-seed", "1", tmp_path / "s.txt", "+1",
                  tmp_path / "a.fa"])
    assert r.returncode == 0, r.stdout + r.stderr
    got = _parse_libsvm((tmp_path / "s.txt").read_text())
    bpp = [gpu_ctx.fold_sample([s.lower()], 200, seed=1)[0] for s in seqs]
    ds = ska.Dataset.from_sequences(seqs, bpp=bpp)
    ref = gpu_ctx.gram(ds, ska.SuStemKernel())
    ref6 = np.array([[float(f"{v:.6g}") for v in row] for row in ref])
    assert got.shape == ref.shape == (4, 4)
    assert np.max(np.abs(got - ref6) / np.maximum(np.abs(ref6), 1e-300)) <= 1e-12
    r = _run_cli(["--no-string", tmp_path / "f.txt", "+1", tmp_path / "a.fa"])
    assert r.returncode == 0, r.stdout + r.stderr
    plain = _parse_libsvm((tmp_path / "f.txt").read_text())
    assert not np.array_equal(plain, got)
    # another seed, another Gram
    r = _run_cli(["--no-string", "--sampling", "200", "--sampling-seed", "2", tmp_path / "t.txt", "+1",
                  tmp_path / "a.fa"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert not np.array_equal(_parse_libsvm((tmp_path / "t.txt").read_text()), got)
