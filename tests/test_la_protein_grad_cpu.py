"""Gradients of the protein local-alignment kernel, host side: the fixture
tests/golden/la_protein_grad.json against the reference's own
compute_gradients (BPLAKernel<double,AAMData>, bpla_kernel.cpp:385-401), the
host path (sk_la_protein_gradients_host) against the fixture bit for bit and
against central differences of its own value, the refusals, the normalised
gradient Gram and optimize_la on a toy set.  No GPU."""
import ctypes as C
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import stem_kernel_amd as ska
from stem_kernel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout absent")
FIELDS = ("value", "d_beta", "d_gap", "d_ext")


def load_fixture():
    """examples, n, kernels (one LAKernel per parameter set) and per set the
    arrays V[n, n] and D[n, n, 4] (alpha slot 0.0) of the reference."""
    with open(os.path.join(ROOT, "tests", "golden", "la_protein_grad.json")) as f:
        fx = json.load(f)
    n = fx["n"] = len(fx["examples"])
    fx["kernels"], fx["V"], fx["D"] = [], [], []
    for p, vals in zip(fx["params"], fx["values"]):
        fx["kernels"].append(ska.LAKernel(gap=float.fromhex(p["gap"]), ext=float.fromhex(p["ext"]),
                                          beta=float.fromhex(p["beta"]), cli_float=False,
                                          score_table=[float.fromhex(t) for t in p["table"]]))
        cols = {k: np.array([float.fromhex(t) for t in vals[k]]).reshape(n, n) for k in FIELDS}
        fx["V"].append(cols["value"])
        fx["D"].append(np.stack([np.zeros((n, n)), cols["d_beta"], cols["d_gap"], cols["d_ext"]], axis=2))
    return fx


def dataset(examples):
    ds = ska.Dataset()
    for k, rows in enumerate(examples):
        ds.add_protein(f"e{k}", rows)
    return ds


def all_pairs(n):
    x, y = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return x.ravel().astype(np.int32), y.ravel().astype(np.int32)


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


@pytest.fixture(scope="module")
def host_results(fixture):
    """The host path over every ordered pair, once per parameter set."""
    ds = dataset(fixture["examples"])
    x, y = all_pairs(fixture["n"])
    return ds, [ska.la_gradients(ds, k, x, y) for k in fixture["kernels"]]


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_la_grad",
                                                  os.path.join(ROOT, "tools", "make_golden_la_grad.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@needs_ref
def test_fixture_is_the_references_output_bit_for_bit(tmp_path):
    gen = _generator()
    exe = gen.build_harness(REF, str(tmp_path))
    with open(os.path.join(ROOT, "tests", "golden", "la_protein_grad.json")) as f:
        fx = json.load(f)
    ex, params = gen.base.examples(), gen.base.parameter_sets()
    assert fx["examples"] == ex
    for p, q in zip(fx["params"], params):
        assert [float.fromhex(p[k]) for k in ("gap", "ext", "beta")] == [q["gap"], q["ext"], q["beta"]]
        assert [float.fromhex(t) for t in p["table"]] == q["table"]
    assert fx["values"] == gen.reference_values(exe, str(tmp_path), ex, params)


def test_fixture_holds_the_cases(fixture):
    n = fixture["n"]
    assert n == 17 and len(fixture["V"]) == 2
    with open(os.path.join(ROOT, "tests", "golden", "la_protein.json")) as f:
        forward = json.load(f)
    assert forward["examples"] == fixture["examples"] and forward["params"] == fixture["params"]
    for s in range(2):
        V, D = fixture["V"][s], fixture["D"][s]
        assert V.shape == (n, n) and np.all(np.isfinite(V)) and np.all(np.isfinite(D))
        # exact zeros where no gap can open or extend; nothing else nearly cancelled
        assert np.sum(D[:, :, 2] == 0) == 34 and np.sum(D[:, :, 3] == 0) == 37
        nz = D[:, :, 1:] != 0
        assert np.all(np.abs(D[:, :, 1:])[nz] >= 1e-3 * np.broadcast_to(V[:, :, None], nz.shape)[nz])
        # the optimizer's model: not operator()'s value, and not symmetric
        K = np.array([float.fromhex(v) for v in forward["values"][s][0]]).reshape(n, n)
        assert np.all(V[3:, 3:] != K[3:, 3:])
        assert np.max(np.abs(V / V.T - 1)) > 1.0


def test_host_path_equals_the_fixture_bit_for_bit(fixture, host_results):
    n = fixture["n"]
    for s, (val, grad) in enumerate(host_results[1]):
        assert np.array_equal(val.reshape(n, n), fixture["V"][s]), s
        assert np.array_equal(grad.reshape(n, n, 4), fixture["D"][s]), s
        assert np.all(grad[:, 0] == 0.0) and not np.any(np.signbit(grad[:, 0]))


def test_host_path_is_thread_count_and_batch_independent(fixture, host_results):
    ds, res = host_results
    x, y = all_pairs(fixture["n"])
    sel = np.array([5, 40, 100, 288, 250])
    for nt in (1, 3):
        v, g = ska.la_gradients(ds, fixture["kernels"][1], x[sel], y[sel], n_threads=nt)
        assert np.array_equal(v, res[1][0][sel]) and np.array_equal(g, res[1][1][sel])


@pytest.mark.parametrize("pair", [(3, 14), (15, 9), (13, 5)])
def test_components_are_derivatives_of_the_value(fixture, host_results, pair):
    """Central differences of the host path's own value, steps 1e-6 (beta) and
    1e-5 (gap, ext), reproduce every nonzero component to 1e-6 relative (the
    same measurement on the reference's function gave about 1e-9)."""
    ds = host_results[0]
    n = fixture["n"]
    for s, kern in enumerate(fixture["kernels"]):
        p = kern.params
        base = dict(beta=p.beta, gap=p.gap, ext=p.ext)
        table = np.array(p.aa_score_table[:])
        grad = host_results[1][s][1].reshape(n, n, 4)[pair]

        def value(**kw):
            k = ska.LAKernel(score_table=table, cli_float=False, **{**base, **kw})
            return ska.la_gradients(ds, k, [pair[0]], [pair[1]])[0][0]

        for q, (name, h) in enumerate((("beta", 1e-6), ("gap", 1e-5), ("ext", 1e-5)), start=1):
            if grad[q] == 0.0:
                continue
            fd = (value(**{name: base[name] + h}) - value(**{name: base[name] - h})) / (2 * h)
            print(f"pair {pair} set {s} d/d{name}: analytic {grad[q]!r} central {fd!r} rel {abs(fd / grad[q] - 1):.3g}")
            assert abs(fd / grad[q] - 1) < 1e-6, (pair, s, name, fd, grad[q])


def _host_call(xs, ys, kernel, x, y):
    x = np.ascontiguousarray(x, dtype=np.int32)
    y = np.ascontiguousarray(y, dtype=np.int32)
    v, g = np.zeros(x.size), np.zeros(4 * x.size)
    p64 = C.POINTER(C.c_double)
    return _lib.lib().sk_la_protein_gradients_host(xs.handle, ys.handle, C.byref(kernel.params),
                                                   x.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   y.ctypes.data_as(C.POINTER(C.c_int32)), x.size, 1,
                                                   v.ctypes.data_as(p64), g.ctypes.data_as(p64))


def test_refusals(fixture):
    ds = dataset(fixture["examples"][:3])
    rna = ska.Dataset()
    rna.add("+1", ["ACGUACGU"], use_bp=False)
    la = ska.LAKernel()
    assert _host_call(ds, ds, la, [0], [2]) == 0
    # a dataset that is not protein, a kind other than SK_AA_LA
    assert _host_call(rna, rna, la, [0], [0]) == -1
    assert _host_call(ds, rna, la, [0], [0]) == -1
    assert _host_call(ds, ds, ska.LAKernel(SW=True), [0], [1]) == -1
    assert _host_call(ds, ds, ska.BPLAKernel(), [0], [1]) == -1
    # an index outside its dataset
    for x, y in (([3], [0]), ([0], [3]), ([-1], [0]), ([0, 1], [1, -1])):
        assert _host_call(ds, ds, la, x, y) == -5
    with pytest.raises(ska.StemKernelError) as e:
        ska.la_gradients(ds, la, [0], [7])
    assert e.value.code == -5
    # the SW kernel has no gradient: refused in Python before any call
    for call in (lambda k: ska.la_gradients(ds, k, [0], [1]), lambda k: ska.la_gradient_gram(ds, k),
                 lambda k: ska.la_auc_objective(ds, k, [1, -1, 1], 2, 1.0), lambda k: ska.optimize_la(ds, [1, -1, 1], k)):
        with pytest.raises(ValueError):
            call(ska.LAKernel(SW=True))
    assert hasattr(ska.Context, "la_gradients") and hasattr(ska.Context, "la_gradient_gram")
    assert hasattr(ska.Context, "la_auc_objective")


def test_symbols_and_shape():
    with open(os.path.join(ROOT, "include", "stem_kernel.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in ("sk_la_protein_gradients", "sk_la_protein_gradients_host", "sk_la_protein_grad_shape",
                 "sk_last_la_protein_grad"):
        assert re.search(r"\b%s\(" % name, header)
        assert name in _lib.SIGNATURES and hasattr(L, name)
    shape = ska.la_grad_shape()
    assert shape["code"] >= 1024 and shape["profile"] >= 1024
    assert shape["code"] % 2 == 0 and shape["profile"] % 2 == 0 and shape["code"] > shape["profile"]


def test_gradient_gram_mirrors_and_normalises(fixture, host_results):
    ds = host_results[0]
    n = fixture["n"]
    kern = fixture["kernels"][0]
    K, G = ska.la_gradient_gram(ds, kern)
    iu = np.triu_indices(n)
    assert np.array_equal(K[iu], fixture["V"][0][iu]) and np.array_equal(K, K.T)
    for q in range(4):
        assert np.array_equal(G[q][iu], fixture["D"][0][:, :, q][iu]) and np.array_equal(G[q], G[q].T)
    assert not np.any(G[0])
    NK, NG = ska.la_gradient_gram(ds, kern, normalize=True)
    assert np.array_equal(np.diag(NK), np.ones(n))
    for q in range(4):
        assert np.array_equal(np.diag(NG[q]), np.zeros(n))
    d = np.diag(K)
    off = ~np.eye(n, dtype=bool)
    assert np.allclose(NK[off], (K / np.sqrt(np.outer(d, d)))[off], rtol=1e-14, atol=0)


def _families():
    """Two synthetic families: 12 noisy copies each of two random ancestors of
    length 30, labels alternating so that every fold holds both."""
    rng = np.random.RandomState(7)
    letters = np.array(list("ARNDCQEGHILKMFPSTWYV"))
    anc = [rng.randint(0, 20, 30) for _ in range(2)]
    seqs, labels = [], []
    for k in range(24):
        fam = k % 2
        s = anc[fam].copy()
        hit = rng.rand(30) < 0.2
        s[hit] = rng.randint(0, 20, int(hit.sum()))
        seqs.append(["".join(letters[s])])
        labels.append(1.0 if fam == 0 else -1.0)
    return dataset(seqs), np.array(labels)


def test_auc_objective_drops_the_alpha_entry():
    ds, labels = _families()
    kern = ska.LAKernel()
    f, g, rec = ska.la_auc_objective(ds, kern, labels, 3, 1.0)
    K, G = ska.la_gradient_gram(ds, kern)
    f2, g2, _ = ska.auc_objective(K, G, labels, 3, 1.0)
    assert f == f2 and g.shape == (4,) and g2.shape == (5,)
    assert g2[1] == 0.0 and np.array_equal(g, g2[[0, 2, 3, 4]]) and len(rec) == 3


def test_optimize_la_on_a_toy_set():
    pytest.importorskip("scipy")
    ds, labels = _families()
    seen = []
    res, best = ska.optimize_la(ds, labels, ska.LAKernel(), C=1.0, n_folds=3, maxfun=4,
                                callback=lambda step, x, f, g: seen.append((x.copy(), f)))
    assert 1 <= len(seen) <= 6
    assert np.array_equal(seen[0][0], [1.0, ska.LAKernel().params.beta, -10.0, -1.0])
    C_, beta, gap, ext = res.x
    assert C_ >= 1e-5 and 1e-3 <= beta <= 0.3 and gap <= 0.0 and ext <= 0.0
    assert res.fun <= seen[0][1]
    p = best.params
    assert (p.beta, p.gap, p.ext) == (beta, gap, ext) and p.kind == _lib.AA_LA
