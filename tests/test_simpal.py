"""Simple palindrome kernel on the GPU (csrc/kernels/simpal.hip; SK_SIMPAL, the
reference's simpal tool) against the restatement tests/simpal_ref.py, which
tests/test_simpal_cpu.py pins to the reference's own code.  The gate is the
project's 1e-6 relative; where the restatement is exactly 0 the GPU is 0.0."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from stem_kernel_amd import shard
from tests import simpal_ref
from tests.test_simpal_cpu import load_fixture, restated

pytestmark = pytest.mark.gpu
TOL = 1e-6  # the project's parity gate


def _check(got, ref, what=""):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got)), what
    zero = ref == 0
    assert np.all(got[zero] == 0.0), what
    rel = np.abs(got[~zero] - ref[~zero]) / ref[~zero]
    worst = float(rel.max()) if rel.size else 0.0
    print(f"simpal {what}: worst relative deviation {worst:.3g} over {rel.size} values, {int(zero.sum())} exact zeros")
    assert worst < TOL, what
    return worst


def _dataset(examples):
    ds = ska.Dataset()
    for k, (keys, dist, w) in enumerate(examples):
        ds.add_palindrome_entries(f"e{k}", keys, dist, w, seed_length=len(keys[0]) if keys else 3)
    return ds


def _random_example(rng, m, s=3, max_d=300):
    """m entries with distinct (key, dist), in map order."""
    pick = rng.choice(4 ** s * max_d, size=m, replace=False) if m else np.zeros(0, np.int64)
    pick.sort()
    keys = ["".join("acgu"[(int(p) // max_d >> 2 * (s - 1 - t)) & 3] for t in range(s)) for p in pick]
    dist = (pick % max_d).astype(np.int32)
    w = rng.uniform(0.01, 1.0, m).astype(np.float32)
    return keys, dist, w


@pytest.fixture(scope="module")
def sized():
    """Examples whose sizes stand on the kernel's boundaries: |P| around the
    wave (64), the x block B = 64 x_block and the y tile T, on either side."""
    T, xb = ska.simpal_shape()
    B = 64 * xb
    xs = [0, 1, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1]
    ys = [0, 1, T - 1, T, T + 1, 2 * T + 3]
    rng = np.random.default_rng(0x51A9A1)
    ex = [_random_example(rng, m) for m in xs + ys]
    n = len(ex)
    R = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            R[i, j] = R[j, i] = simpal_ref.kernel_vec(ex[i], ex[j], 1)
    return dict(ex=ex, ds=_dataset(ex), R=R, n=n, nx=len(xs), sizes=xs + ys)


def test_sizes_all_ordered_pairs(gpu_ctx, sized):
    """Every size on the x side against every size on the y side, and the
    reverse, through sk_pairs in one call."""
    n = sized["n"]
    x, y = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    got = gpu_ctx.pairs(sized["ds"], ska.SimpalKernel(), x, y).reshape(n, n)
    _check(got, sized["R"], "sizes, sk_pairs")
    tm = gpu_ctx.last_timing()
    assert tm["launches"] == 1 and tm["cells"] == float(sum(sized["sizes"])) ** 2  # the terms


def test_sizes_as_a_gram(gpu_ctx, sized):
    g = gpu_ctx.gram(sized["ds"], ska.SimpalKernel())
    assert np.array_equal(g, g.T)
    _check(g, sized["R"], "sizes, Gram")


@pytest.mark.parametrize("s", [1, 3, 16, 17, 32])
def test_keys_and_tolerances(gpu_ctx, s):
    """Single-entry examples whose keys differ from the base key in the first
    letter only, the last letter only, and in exactly m letters for every m a
    tolerance in {-1, 0, 1, s} separates (m = tolerance and tolerance + 1)."""
    rng = np.random.default_rng(100 + s)
    base = "".join(rng.choice(list("acgu"), s))
    other = lambda c: "acgu"[("acgu".index(c) + 1 + int(rng.integers(0, 3))) % 4]

    def variant(pos):
        k = list(base)
        for p in pos:
            k[p] = other(k[p])
        return "".join(k)

    counts = sorted({m for m in (0, 1, 2, s - 1, s, s // 2) if 0 <= m <= s})
    keys = [base, variant([0]), variant([s - 1])]
    keys += [variant(rng.choice(s, m, replace=False)) for m in counts]
    # 2-bit codes that differ in the high bit only, the low bit only, and both
    keys += [base.replace(base[0], c) for c in "acgu"]
    ex = [([k], np.array([3 + i % 3], np.int32), np.array([0.5 + 0.01 * i], np.float32)) for i, k in enumerate(keys)]
    ds = _dataset(ex)
    n = len(ex)
    x, y = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    for tol in sorted({-1, 0, 1, s}):
        got = gpu_ctx.pairs(ds, ska.SimpalKernel(tolerance=tol), x, y)
        ref = np.array([simpal_ref.kernel_seq(ex[a], ex[b], tol) for a, b in zip(x, y)])
        assert (ref == 0).any() or tol in (-1, s)
        _check(got, ref, f"keys s={s} tolerance={tol}")


def test_exponent(gpu_ctx):
    """e^-|d| equals libm's within the gate, is exactly 0 from |d| = 746 on,
    and is never inf or NaN however far apart the dists."""
    d = [0, 1, 297, 700, 746, 5000, 2 ** 30]
    ex = [(["acg"], np.array([0], np.int32), np.array([1.0], np.float32))]
    ex += [(["acg"], np.array([v], np.int32), np.array([0.75], np.float32)) for v in d]
    # a mixed example whose dists span 0 to 2^30
    mk = ["aaa", "acg", "acg", "acg", "acu", "gcg", "ucg", "uuu", "uuu"]
    md = np.array([2 ** 30, 0, 745, 2 ** 30 - 1, 300, 746, 5000, 1, 2 ** 30], np.int32)
    mixed = simpal_ref_sorted(mk, md, np.linspace(0.1, 0.9, 9).astype(np.float32))
    ex.append(mixed)
    ds = _dataset(ex)
    n = len(ex)
    x, y = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    got = gpu_ctx.pairs(ds, ska.SimpalKernel(), x, y).reshape(n, n)
    ref = np.array([simpal_ref.kernel_seq(ex[a], ex[b], 1) for a, b in zip(x, y)]).reshape(n, n)
    for j, v in enumerate(d, start=1):
        assert (ref[0, j] == 0.0) == (v >= 746)
        assert (got[0, j] == 0.0) == (v >= 746) and got[j, 0] == got[0, j]
    assert ref[n - 1, n - 1] > 0 and np.isfinite(got[n - 1, n - 1])
    _check(got, ref, "exponent")


def simpal_ref_sorted(keys, dist, w):
    order = sorted(range(len(keys)), key=lambda i: (keys[i], int(dist[i])))
    return [keys[i] for i in order], np.asarray(dist)[order], np.asarray(w)[order]


def test_bits_do_not_depend_on_the_batch(gpu_ctx, sized):
    """A pair alone, inside the Gram and inside a 2-way split of the Gram
    (sk_shard_cells lists): the same bits, in async mode too."""
    import torch
    ds, n = sized["ds"], sized["n"]
    kern = ska.SimpalKernel()
    g = gpu_ctx.gram(ds, kern)
    for i, j in ((3, 15), (9, 15), (9, 9), (14, 15), (0, 7), (12, 13), (8, 14)):
        assert gpu_ctx.pairs(ds, kern, [i], [j])[0] == g[i, j]
    iu, ju = (a.astype(np.int32) for a in np.triu_indices(n))
    perm = np.random.default_rng(1).permutation(iu.size)
    assert np.array_equal(gpu_ctx.pairs(ds, kern, iu[perm], ju[perm]), g[iu[perm], ju[perm]])
    cells = [shard.rank_pairs(n, 2, r) for r in range(2)]
    parts = [gpu_ctx.pairs(ds, kern, x, y) for x, y in cells]
    assert np.array_equal(shard.assemble(parts, n, 2), g)
    assert np.array_equal(shard.assemble(parts, n, 2, normalize=True), gpu_ctx.gram(ds, kern, normalize=True),
                          equal_nan=True)
    gpu_ctx.set_async(True)
    try:
        outs = []
        for x, y in cells + [(np.array([9], np.int32), np.array([15], np.int32))]:
            o = torch.full((x.size,), float("nan"), dtype=torch.float64, device="cuda:0")
            gpu_ctx.pairs_device(ds, kern, x.copy(), y.copy(), o.data_ptr())
            outs.append(o)
        torch.cuda.synchronize()
        gpu_ctx.sync_timing()
        assert gpu_ctx.last_timing()["launches"] == 3 and gpu_ctx.last_launch_ms()["launches"] >= 1
        for o, p in zip(outs, parts):
            assert np.array_equal(o.cpu().numpy(), p)
        assert outs[2].cpu().numpy()[0] == g[9, 15]
    finally:
        gpu_ctx.set_async(False)


@pytest.fixture(scope="module")
def fx():
    f = load_fixture()
    idx = [k for k, e in enumerate(f["examples"]) if e["set"] == "s3"]
    ex = [f["examples"][k] for k in idx]
    ds = ska.Dataset()
    for e in ex:
        ds.add_palindromes("+1", e["seq"], e["bpp"], e["seed_length"], e["min_loop"], e["max_dist"])
    ent = [restated(e) for e in ex]
    return dict(ex=ex, ds=ds, ent=ent, n=len(ex), K=simpal_ref.gram(ent, 1, kernel=simpal_ref.kernel_seq))


def test_gram_of_the_fixture_sequences(gpu_ctx, fx):
    kern = ska.SimpalKernel()
    g = gpu_ctx.gram(fx["ds"], kern)
    assert np.array_equal(g, g.T)
    _check(g, fx["K"], "fixture Gram")
    # -n: an example without palindromes has a zero diagonal; its row and
    # column are NaN and its diagonal cell 1, as in the reference
    # (common/kernel_matrix.cpp:560-571)
    gn = gpu_ctx.gram(fx["ds"], kern, normalize=True)
    want = simpal_ref.gram(fx["ent"], 1, normalize=True, kernel=simpal_ref.kernel_seq)
    empty = np.array([len(e[0]) == 0 for e in fx["ent"]])
    assert empty.any() and not empty.all()
    off = ~np.eye(fx["n"], dtype=bool)
    assert np.array_equal(np.isnan(gn), np.isnan(want))
    assert np.all(np.isnan(gn[empty[:, None] & off])) and np.all(np.diag(gn) == 1.0)
    ok = ~np.isnan(want)
    _check(gn[ok], want[ok], "fixture Gram -n")
    # every tolerance of the fixture against the restatement
    for tol in (-1, 0, 3):
        _check(gpu_ctx.gram(fx["ds"], ska.SimpalKernel(tolerance=tol)),
               simpal_ref.gram(fx["ent"], tol), f"fixture Gram tolerance={tol}")


def test_test_row_diagonal_and_test_matrix(gpu_ctx, fx):
    kern = ska.SimpalKernel()
    K, ds = fx["K"], fx["ds"]
    _check(gpu_ctx.diagonal(ds, kern), np.diag(K), "diagonal")
    sv = np.array([3, 4, 5, 7], np.int32)
    _check(gpu_ctx.diagonal(ds, kern, sv)[sv], np.diag(K)[sv], "diagonal sv_index")
    t = 5
    row, self_ = gpu_ctx.test_row(ds, t, ds, kern, self_value=True)
    _check(row, K[:, t], "test row")  # out[i] = K(train[i], test[t])
    assert abs(self_ / K[t, t] - 1.0) < TOL
    row = gpu_ctx.test_row(ds, t, ds, kern, sv_index=sv)
    row = row[0] if isinstance(row, tuple) else row
    _check(row[sv], K[sv, t], "test row sv_index")
    out, selfs = gpu_ctx.test_matrix(ds, ds, kern, norm_test=True)
    _check(out, K.T, "test matrix")
    _check(selfs, np.diag(K), "test matrix self values")


def test_folded_equals_add_palindromes_of_the_fold(gpu_ctx, fx):
    """add_palindromes_folded = add_palindromes fed sk_fold_mccaskill's output
    (no claim against ViennaRNA, as for every folded path)."""
    seqs = [e["seq"] for e in fx["ex"] if len(e["seq"]) >= 7][:6]
    a = ska.Dataset()
    a.add_palindromes_folded(gpu_ctx, seqs, labels=[f"l{k}" for k in range(len(seqs))], threads=2)
    bpps = gpu_ctx.fold([s.lower() for s in seqs], no_gu=True)
    b = ska.Dataset()
    for s, p in zip(seqs, bpps):
        b.add_palindromes("+1", s, p)
    assert len(a) == len(b) == len(seqs) and a.label(1) == "l1"
    some = 0
    for i in range(len(seqs)):
        ka, da, wa = a.palindromes(i)
        kb, db, wb = b.palindromes(i)
        assert ka == kb and np.array_equal(da, db) and np.array_equal(wa.view(np.uint32), wb.view(np.uint32))
        some += int((wa > 0).sum())
    assert some > 0
    assert np.array_equal(gpu_ctx.gram(a, ska.SimpalKernel()), gpu_ctx.gram(b, ska.SimpalKernel()))


def test_kinds_and_datasets_do_not_cross(gpu_ctx, fx):
    rna = ska.Dataset()
    rna.add("+1", ["ACGUACGU"], use_bp=False)
    with pytest.raises(ska.StemKernelError) as e:
        gpu_ctx.pairs(rna, ska.SimpalKernel(), [0], [0])
    assert e.value.code == -1 and "palindrome" in str(e.value)
    for kern in (ska.StringKernel(), ska.BPLAKernel(noBP=True), ska.LAKernel(), ska.StemKernel4D()):
        with pytest.raises(ska.StemKernelError) as e:
            gpu_ctx.pairs(fx["ds"], kern, [3], [4])
        assert e.value.code == -1 and "palindrome" in str(e.value)
    with pytest.raises(ska.StemKernelError) as e:
        gpu_ctx.bpla_gradients(fx["ds"], ska.BPLAKernel(), [3], [4])
    assert e.value.code == -1 and "palindrome" in str(e.value)
    prot = ska.Dataset()
    prot.add_protein("+1", ["MKV"])
    with pytest.raises(ska.StemKernelError) as e:
        gpu_ctx.pairs(prot, ska.SimpalKernel(), [0], [0])
    assert e.value.code == -1
    # the tolerance is an integer
    kern = ska.SimpalKernel()
    kern.params.mismatch = 0.5
    with pytest.raises(ska.StemKernelError) as e:
        gpu_ctx.pairs(fx["ds"], kern, [3], [4])
    assert e.value.code == -1 and "integer" in str(e.value)
    # a test set of another seed_length
    two = ska.Dataset()
    two.add_palindrome_entries("+1", ["ac"], [3], [1.0])
    with pytest.raises(ska.StemKernelError) as e:
        gpu_ctx.test_row(two, 0, fx["ds"], ska.SimpalKernel())
    assert e.value.code == -1


@pytest.mark.parametrize("fold,tolerance,normalize", [("synthetic", 1, 0), ("engine", 0, 1)])
def test_simpal_dropin_matches_engine(gpu_ctx, fx, tmp_path, fold, tolerance, normalize):
    """The reference-shaped simpal main over the compat header gives the
    engine's matrices bit for bit, from FASTA files."""
    import subprocess

    from tests.test_simpal_cpu import build_dropin
    exe = build_dropin(tmp_path)
    seqs = [e["seq"] for e in fx["ex"] if e["min_loop"] == 3 and e["max_dist"] == 300 and len(e["seq"]) >= 7]
    train, test = seqs[:4], seqs[4:6]
    for name, ss in (("tr.fa", train), ("te.fa", test)):
        with open(tmp_path / name, "w") as f:
            for k, s in enumerate(ss):
                f.write(f">s{k}\n{s}\n")

    def dataset(ss):
        ds = ska.Dataset()
        if fold == "synthetic":
            for s in ss:
                ds.add_palindromes("+1", s)
        else:
            ds.add_palindromes_folded(gpu_ctx, ss)
        return ds

    def run(*files):
        out = subprocess.run([exe, str(tmp_path / "g.txt"), str(tolerance), str(normalize), fold,
                              *[str(tmp_path / f) for f in files]],
                             check=True, capture_output=True, text=True, timeout=300).stdout.splitlines()
        r, c = (int(v) for v in out[0].split())
        m = np.array([[float(v) for v in out[1 + i].split()] for i in range(r)]).reshape(r, c)
        return m, out[1 + r:]

    kern = ska.SimpalKernel(tolerance=tolerance)
    dtr, dte = dataset(train), dataset(test)
    m, rest = run("tr.fa")
    assert np.array_equal(m, gpu_ctx.gram(dtr, kern, normalize=bool(normalize)), equal_nan=True)
    assert float(rest[0].split()[1]) == gpu_ctx.gram(dtr, kern)[0, 1]  # Kernel::operator() on one pair
    m, rest = run("tr.fa", "te.fa")
    want, selfs = gpu_ctx.test_matrix(dte, dtr, kern, norm_test=True, normalize=bool(normalize))
    assert np.array_equal(m, want, equal_nan=True)
    assert [float(l.split()[1]) for l in rest[:len(test)]] == list(selfs)
    text = (tmp_path / "g.txt").read_text().splitlines()
    assert len(text) == len(test) and text[0].startswith("-1 0:1 1:")
