"""Protein local-alignment kernel on the GPU (csrc/kernels/la_protein.hip;
SK_AA_LA / SK_AA_LA_SW, the reference's la_kernel) against the fixture made
from the reference's own code (tests/golden/la_protein.json) and, for random
inputs, against its bit-exact numpy restatement (tests/la_ref.py)."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from tests import la_ref
from tests.test_la_protein_cpu import load_fixture

pytestmark = pytest.mark.gpu
TOL = 1e-6  # the project's parity gate


@pytest.fixture(scope="module")
def fx():
    f = load_fixture()
    ds = ska.Dataset()
    for k, rows in enumerate(f["examples"]):
        ds.add_protein(f"e{k}", rows)
    f["ds"] = ds
    return f


def _kernel(p, SW):
    return ska.LAKernel(SW=SW, gap=p["gap"], ext=p["ext"], beta=p["beta"], score_table=p["table"], cli_float=False)


def _rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.abs(np.where(ref == 0, 1.0, ref))))


@pytest.mark.parametrize("SW", [False, True])
@pytest.mark.parametrize("pset", [0, 1])
def test_pairs_match_the_reference_fixture(gpu_ctx, fx, pset, SW):
    n = fx["n"]
    x, y = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    got = gpu_ctx.pairs(fx["ds"], _kernel(fx["params"][pset], SW), x, y).reshape(n, n)
    ref = fx["K"][pset][int(SW)]
    # both kernels ran in this one call: single sequences pair on the code
    # kernel, every pair with a mixed-column alignment on the profile kernel
    assert gpu_ctx.last_la_protein() == dict(code=True, profile=True)
    coded = np.array([len(r) == 1 or len(set(r)) == 1 for r in fx["examples"]])
    code = coded[:, None] & coded[None, :]
    print(f"la_protein set {pset} SW={SW}: worst relative error code path {_rel(got[code], ref[code]):.3g}, "
          f"profile path {_rel(got[~code], ref[~code]):.3g}")
    assert np.all(np.isfinite(got))
    assert _rel(got, ref) < TOL
    if SW and pset == 0:
        assert np.array_equal(got, ref)  # max-plus over exactly representable sums
    elif SW:
        assert _rel(got, ref) <= 1e-12


def test_identical_rows_equal_the_single_row(gpu_ctx, fx):
    """Three identical rows score what the row scores alone (counts 3 against
    1: the factor cancels in LAScore), against every example in either role:
    single sequences (code kernel) and alignments (profile kernel)."""
    n = fx["n"]
    same, single = 16, 5
    assert fx["examples"][same] == [fx["examples"][single][0]] * 3
    others = np.arange(n)
    kern = _kernel(fx["params"][0], False)
    a = gpu_ctx.pairs(fx["ds"], kern, np.full(n, same), others)
    b = gpu_ctx.pairs(fx["ds"], kern, np.full(n, single), others)
    assert gpu_ctx.last_la_protein() == dict(code=True, profile=True)
    assert _rel(a, b) <= 1e-12
    a = gpu_ctx.pairs(fx["ds"], kern, others, np.full(n, same))
    b = gpu_ctx.pairs(fx["ds"], kern, others, np.full(n, single))
    assert _rel(a, b) <= 1e-12
    assert abs(a[same] / fx["K"][0][0][single, single] - 1.0) <= 1e-12


@pytest.mark.parametrize("SW", [False, True])
def test_gram(gpu_ctx, fx, SW):
    n = fx["n"]
    kern = _kernel(fx["params"][0], SW)
    ref = fx["K"][0][int(SW)]
    up = np.triu_indices(n)
    g = gpu_ctx.gram(fx["ds"], kern)
    assert np.array_equal(g, g.T)  # K(x, y) for x <= y, mirrored
    assert _rel(g[up], ref[up]) < TOL
    gn = gpu_ctx.gram(fx["ds"], kern, normalize=True)
    assert np.array_equal(gn, gn.T)
    d = np.diag(ref)
    ok = d > 0  # (SW: the length-1 residue can score 0 against itself; NaN propagates as in the reference)
    assert np.all(np.diag(gn) == 1.0)
    want = ref / np.sqrt(d[:, None] * d[None, :])
    m = ok[:, None] & ok[None, :]
    m &= ~np.eye(n, dtype=bool)
    m &= np.triu(np.ones((n, n), bool))
    assert m.sum() > n and _rel(gn[m], want[m]) < TOL


def test_test_row_and_diagonal(gpu_ctx, fx):
    n = fx["n"]
    kern = _kernel(fx["params"][1], False)
    ref = fx["K"][1][0]
    assert _rel(gpu_ctx.diagonal(fx["ds"], kern), np.diag(ref)) < TOL
    sv = np.array([0, 3, 14, 16], np.int32)
    d = gpu_ctx.diagonal(fx["ds"], kern, sv)
    assert _rel(d[sv], np.diag(ref)[sv]) < TOL
    t = 15
    row, self_ = gpu_ctx.test_row(fx["ds"], t, fx["ds"], kern, self_value=True)
    assert _rel(row, ref[:, t]) < TOL  # out[i] = K(train[i], test[t])
    assert abs(self_ / ref[t, t] - 1.0) < TOL
    out, selfs = gpu_ctx.test_matrix(fx["ds"], fx["ds"], kern, norm_test=True)
    assert _rel(out, ref.T) < TOL and _rel(selfs, np.diag(ref)) < TOL


@pytest.mark.parametrize("seed", range(8))
def test_random_sweep_matches_the_restatement(gpu_ctx, seed):
    rng = np.random.default_rng(0x1A0000 + seed)
    letters = np.array(list(la_ref.AA_LETTERS + "-"))
    ex = []
    for _ in range(6):
        L = int(rng.integers(1, 151))
        rows = 1 if rng.random() < 0.5 else int(rng.integers(2, 6))
        base = rng.integers(0, 20, L)
        al = []
        for _r in range(rows):
            r = base.copy()
            mut = rng.random(L) < (0.0 if rows == 1 else 0.3)
            r[mut] = rng.integers(0, 24, int(mut.sum()))
            al.append("".join(letters[r]))
        ex.append(al)
    table = rng.uniform(-4.0, 6.0, (23, 23))
    gap, ext, beta = rng.uniform(-12.0, -2.0), rng.uniform(-2.0, -0.1), rng.uniform(0.05, 0.3)
    ds = ska.Dataset()
    for rows in ex:
        ds.add_protein("+1", rows)
    cnt = [la_ref.counts(r) for r in ex]
    x, y = (a.ravel() for a in np.meshgrid(np.arange(6), np.arange(6), indexing="ij"))
    for SW in (False, True):
        kern = ska.LAKernel(SW=SW, gap=gap, ext=ext, beta=beta, score_table=table, cli_float=False)
        got = gpu_ctx.pairs(ds, kern, x, y)
        ref = np.array([la_ref.kernel_profiles(cnt[a], cnt[b], table, gap, ext, beta, sw=SW) for a, b in zip(x, y)])
        assert np.all(np.isfinite(ref))
        assert _rel(got, ref) < TOL, (seed, SW)


def test_overflow_is_inf_and_leaves_its_neighbour_alone(gpu_ctx):
    ex = ["W" * 700, "MKVLAAGIWY", "HQRSTWWY"]
    ds = ska.Dataset()
    for s in ex:
        ds.add_protein("+1", [s])
    kern = ska.LAKernel()
    p = kern.params
    ref = [la_ref.kernel(ex[a], ex[b], list(p.aa_score_table), p.gap, p.ext, p.beta) for a, b in ((0, 0), (1, 2))]
    assert ref[0] == np.inf and np.isfinite(ref[1])
    got = gpu_ctx.pairs(ds, kern, [1, 0, 1], [2, 0, 2])
    assert got[1] == np.inf
    assert abs(got[0] / ref[1] - 1.0) < TOL and got[2] == got[0]


def test_one_residue_past_the_length_limit_is_unsupported(gpu_ctx):
    """The code kernel holds a y of up to 6,366 residues in one wave's LDS."""
    ds = ska.Dataset()
    ds.add_protein("+1", ["A" * 6367])
    ds.add_protein("+1", ["ACDEFGHIKL"])
    kern = ska.LAKernel(SW=True)
    with pytest.raises(ska.StemKernelError) as e:
        gpu_ctx.pairs(ds, kern, [1], [0])
    assert e.value.code == -6 and "too long" in str(e.value)
    assert gpu_ctx.last_timing()["launches"] == 0  # no launch was made
    # the limit is the y example's: the long one as x is fine
    assert gpu_ctx.pairs(ds, kern, [0], [1])[0] == 4.0
    # and a y of exactly the limit runs (one wave per workgroup, 163,808 B of LDS)
    ds2 = ska.Dataset()
    ds2.add_protein("+1", ["A" * 6366])
    ds2.add_protein("+1", ["ACDEFGHIKL"])
    assert gpu_ctx.pairs(ds2, kern, [1], [0])[0] == 4.0
    assert gpu_ctx.last_la_protein() == dict(code=True, profile=False)


def test_kinds_and_datasets_do_not_cross(gpu_ctx, fx):
    rna = ska.Dataset()
    rna.add("+1", ["ACGUACGU"], use_bp=False)
    with pytest.raises(ska.StemKernelError) as e:
        gpu_ctx.pairs(rna, ska.LAKernel(), [0], [0])
    assert e.value.code == -1 and "protein" in str(e.value)
    with pytest.raises(ska.StemKernelError) as e:
        gpu_ctx.pairs(fx["ds"], ska.BPLAKernel(noBP=True), [0], [0])
    assert e.value.code == -1 and "protein" in str(e.value)


@pytest.mark.parametrize("sw,normalize", [(0, 0), (1, 1)])
def test_la_dropin_matches_engine(gpu_ctx, fx, tmp_path, sw, normalize):
    """The reference-shaped la_kernel main over the compat header gives the
    engine's Gram bit for bit, from a FASTA file of protein sequences."""
    import subprocess

    from tests.test_la_protein_cpu import build_dropin
    exe = build_dropin(tmp_path)
    seqs = [fx["examples"][i][0] for i in (2, 4, 6, 13)]
    with open(tmp_path / "tr.fa", "w") as f:
        for k, s in enumerate(seqs):
            f.write(f">s{k}\n{s}\n")
    out = subprocess.run([exe, str(tmp_path / "g.txt"), str(sw), str(normalize), str(tmp_path / "tr.fa")],
                         check=True, capture_output=True, text=True, timeout=300).stdout.splitlines()
    assert out[0].startswith("example 0: 3 columns, 1 rows, char2aa('w') = 17")
    ds = ska.Dataset()
    for s in seqs:
        ds.add_protein("+1", [s])
    kern = ska.LAKernel(SW=bool(sw))
    g = gpu_ctx.gram(ds, kern, normalize=bool(normalize))
    got = np.array([[float(v) for v in out[4 + i].split()] for i in range(4)])
    assert np.array_equal(got, g)
    assert float(out[8].split()[1]) == gpu_ctx.gram(ds, kern)[0, 1]


def test_profile_kernel_length_limit(gpu_ctx):
    """The profile kernel holds a y alignment of up to 1,326 columns."""
    ds = ska.Dataset()
    ds.add_protein("+1", ["A" * 1327, "C" * 1327])
    ds.add_protein("+1", ["ACD"])
    kern = ska.LAKernel(SW=True)
    with pytest.raises(ska.StemKernelError) as e:
        gpu_ctx.pairs(ds, kern, [1], [0])
    assert e.value.code == -6 and "too long" in str(e.value)
    assert gpu_ctx.last_timing()["launches"] == 0
    # as x it is fine: every column scores (t[A][b] + t[C][b]) / 2, best path A, C = 2 + 4.5
    assert gpu_ctx.pairs(ds, kern, [0], [1])[0] == 6.5
    assert gpu_ctx.last_la_protein() == dict(code=False, profile=True)
    # a y of exactly the limit runs
    ds2 = ska.Dataset()
    ds2.add_protein("+1", ["A" * 1326, "C" * 1326])
    ds2.add_protein("+1", ["ACD"])
    assert gpu_ctx.pairs(ds2, kern, [1], [0])[0] == 6.5


def test_async_calls_equal_sync(gpu_ctx, fx):
    """sk_set_async: the calls' inputs (pairs, table) are staged, the results
    equal the synchronous calls' bit for bit."""
    import gc

    import torch
    kern = _kernel(fx["params"][1], False)
    rng = np.random.default_rng(5)
    calls = [(rng.integers(0, fx["n"], 40 + 9 * k).astype(np.int32), rng.integers(0, fx["n"], 40 + 9 * k).astype(np.int32))
             for k in range(6)]
    ref = [gpu_ctx.pairs(fx["ds"], kern, x, y) for x, y in calls]
    gpu_ctx.set_async(True)
    try:
        outs = []
        for x, y in calls:  # more calls than the ring of timing sets (4)
            o = torch.full((x.size,), float("nan"), dtype=torch.float64, device="cuda:0")
            xa, ya = x.copy(), y.copy()
            gpu_ctx.pairs_device(fx["ds"], kern, xa, ya, o.data_ptr())
            del xa, ya
            gc.collect()
            outs.append(o)
        torch.cuda.synchronize()
        gpu_ctx.sync_timing()
        for o, r in zip(outs, ref):
            assert np.array_equal(o.cpu().numpy(), r)
    finally:
        gpu_ctx.set_async(False)
    assert np.array_equal(gpu_ctx.pairs(fx["ds"], kern, *calls[0]), ref[0])
