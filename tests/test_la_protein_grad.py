"""Gradients of the protein local-alignment kernel on the GPU
(csrc/kernels/la_protein_grad.hip, sk_la_protein_gradients): every ordered
pair of tests/golden/la_protein_grad.json, the reference's own
compute_gradients, within the project's 1e-6 gate (tests.helpers.rel_err, as
tests/test_bpla_grad.py) and with its exact zeros; the host path at the y
limits of both kernels and on a many-strip x; the refusal past the limit;
determinism; and the optimizer step composed from the parts."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from tests.helpers import rel_err
from tests.test_la_protein_grad_cpu import all_pairs, dataset, load_fixture

pytestmark = pytest.mark.gpu
NAMES = ("value", "d_beta", "d_gap", "d_ext")


@pytest.fixture(scope="module")
def fixture():
    fx = load_fixture()
    fx["ds"] = dataset(fx["examples"])
    fx["x"], fx["y"] = all_pairs(fx["n"])
    return fx


@pytest.fixture(scope="module")
def gpu_results(fixture, gpu_ctx):
    """Every ordered pair under every parameter set: one call per set."""
    out = []
    for kern in fixture["kernels"]:
        val, grad = gpu_ctx.la_gradients(fixture["ds"], kern, fixture["x"], fixture["y"])
        out.append((val, grad, gpu_ctx.last_la_protein_grad(), gpu_ctx.last_launch_ms()["launches"]))
    return out


def assert_matches(val, grad, ref_val, ref_grad, what):
    """The zero rule and the 1e-6 gate; prints the worst deviation per component."""
    ref_grad = np.asarray(ref_grad).reshape(-1, 4)
    grad = np.asarray(grad).reshape(-1, 4)
    assert np.all(grad[:, 0] == 0.0) and not np.any(np.signbit(grad[:, 0]))
    errs = [rel_err(val, np.asarray(ref_val).ravel())]
    for q in (1, 2, 3):
        zero = ref_grad[:, q] == 0.0
        assert np.all(grad[zero, q] == 0.0), (what, NAMES[q])
        errs.append(rel_err(grad[~zero, q], ref_grad[~zero, q]) if np.any(~zero) else 0.0)
    print(what + ": worst relative deviation " + ", ".join(f"{n} {e:.3g}" for n, e in zip(NAMES, errs)))
    for n, e in zip(NAMES, errs):
        assert e < 1e-6, (what, n, e)


def test_fixture_pairs(fixture, gpu_results):
    n = fixture["n"]
    for s, (val, grad, ran, launches) in enumerate(gpu_results):
        assert ran == dict(code=True, profile=True) and launches == 2
        assert_matches(val, grad, fixture["V"][s], fixture["D"][s], f"fixture set {s}")
    # the single sequences ran the code kernel, the alignments the profile kernel
    assert n == 17


def _random_protein(rng, length):
    return "".join(np.array(list("ARNDCQEGHILKMFPSTWYV"))[rng.randint(0, 20, length)])


def _gpu_and_host(gpu_ctx, rows_x, rows_y, kern, what, want):
    ds = dataset([rows_x, rows_y])
    val, grad = gpu_ctx.la_gradients(ds, kern, [0], [1])
    assert gpu_ctx.last_la_protein_grad() == want
    hv, hg = ska.la_gradients(ds, kern, [0], [1])
    assert_matches(val, grad, hv, hg, what)


def test_y_at_the_limit_of_each_path_equals_the_host_path(gpu_ctx):
    rng = np.random.RandomState(11)
    shape = ska.la_grad_shape()
    kern = ska.LAKernel()
    y = _random_protein(rng, shape["code"])
    _gpu_and_host(gpu_ctx, ["WCH"], [y], kern, f"code kernel, y of {shape['code']}", dict(code=True, profile=False))
    y = _random_protein(rng, shape["profile"])
    y2 = y[:40] + "-" + y[41:500] + _random_protein(rng, shape["profile"] - 500)
    _gpu_and_host(gpu_ctx, ["WCH"], [y, y2], kern, f"profile kernel, y of {shape['profile']}",
                  dict(code=False, profile=True))


def test_many_strips_of_x_against_one_column_equal_the_host_path(gpu_ctx):
    rng = np.random.RandomState(12)
    kern = ska.LAKernel()
    x = _random_protein(rng, 257)
    _gpu_and_host(gpu_ctx, [x], ["W"], kern, "code kernel, x of 257, y of 1", dict(code=True, profile=False))
    x2 = x[:100] + "-" + _random_protein(rng, 156)
    _gpu_and_host(gpu_ctx, [x, x2], ["W"], kern, "profile kernel, x of 257, y of 1", dict(code=False, profile=True))


def test_a_y_over_the_limit_is_refused_before_any_launch(gpu_ctx):
    rng = np.random.RandomState(13)
    shape = ska.la_grad_shape()
    kern = ska.LAKernel()
    y = _random_protein(rng, shape["code"] + 1)
    for rows_y in ([y], [y[:shape["profile"] + 1], "-" + y[1:shape["profile"] + 1]]):
        ds = dataset([["WCH"], rows_y])
        with pytest.raises(ska.StemKernelError) as e:
            gpu_ctx.la_gradients(ds, kern, [0, 0], [0, 1])
        assert e.value.code == -6
        assert gpu_ctx.last_launch_ms()["launches"] == 0
        assert gpu_ctx.last_la_protein_grad() == dict(code=False, profile=False)
        # the x length is not limited
        val, _ = gpu_ctx.la_gradients(ds, kern, [1], [0])
        assert np.isfinite(val[0]) and gpu_ctx.last_launch_ms()["launches"] == 1
    # the other refusals, as on the host path, with nothing launched
    rna = ska.Dataset()
    rna.add("+1", ["ACGUACGU"], use_bp=False)
    gpu_ctx.upload(rna)
    assert _gpu_call(gpu_ctx, ds, ska.LAKernel(SW=True), [0], [0]) == -1
    assert _gpu_call(gpu_ctx, ds, ska.BPLAKernel(), [0], [0]) == -1
    assert _gpu_call(gpu_ctx, rna, kern, [0], [0]) == -1
    assert _gpu_call(gpu_ctx, ds, kern, [0], [2]) == -5
    assert gpu_ctx.last_launch_ms()["launches"] == 0
    with pytest.raises(ValueError):
        gpu_ctx.la_gradients(ds, ska.LAKernel(SW=True), [0], [0])


def _gpu_call(ctx, ds, kernel, x, y):
    """sk_la_protein_gradients itself (the Python layer refuses the SW kernel before it)."""
    import ctypes as C
    x = np.ascontiguousarray(x, dtype=np.int32)
    y = np.ascontiguousarray(y, dtype=np.int32)
    v, g = np.zeros(x.size), np.zeros(4 * x.size)
    p64 = C.POINTER(C.c_double)
    return ska.lib().sk_la_protein_gradients(ctx.handle, ds.handle, ds.handle, C.byref(kernel.params),
                                             x.ctypes.data_as(C.POINTER(C.c_int32)),
                                             y.ctypes.data_as(C.POINTER(C.c_int32)), x.size,
                                             v.ctypes.data_as(p64), g.ctypes.data_as(p64))


def test_a_pair_has_the_same_bits_alone_in_a_batch_and_in_the_reversed_batch(fixture, gpu_ctx, gpu_results):
    x, y = fixture["x"], fixture["y"]
    n = fixture["n"]
    kern = fixture["kernels"][1]
    val, grad = gpu_results[1][0], gpu_results[1][1]
    rval, rgrad = gpu_ctx.la_gradients(fixture["ds"], kern, x[::-1].copy(), y[::-1].copy())
    assert np.array_equal(rval[::-1], val) and np.array_equal(rgrad[::-1], grad)
    for a, b in ((12, 11), (15, 14), (9, 15), (0, 0)):  # code, profile, sequence x alignment, one cell
        k = a * n + b
        v1, g1 = gpu_ctx.la_gradients(fixture["ds"], kern, [a], [b])
        assert v1[0] == val[k] and np.array_equal(g1[0], grad[k]), (a, b)


def test_auc_objective_is_the_composition_bit_for_bit(gpu_ctx):
    from tests.test_la_protein_grad_cpu import _families
    ds, labels = _families()
    kern = ska.LAKernel()
    f, g, rec = gpu_ctx.la_auc_objective(ds, kern, labels, 3, 2.0, normalize=True)
    assert np.isfinite(f) and g.shape == (4,) and len(rec) == 3
    K, G = gpu_ctx.la_gradient_gram(ds, kern, normalize=True)
    f2, g2, _ = ska.auc_objective(K, G, labels, 3, 2.0, ctx=gpu_ctx)
    bits = lambda a: np.asarray(a, dtype=np.float64).view(np.uint64)  # noqa: E731
    assert bits([f])[0] == bits([f2])[0]
    g2 = np.delete(g2, 1)
    nan = np.isnan(g2)
    assert np.array_equal(np.isnan(g), nan) and np.array_equal(bits(g)[~nan], bits(g2)[~nan])
    assert -3.0 <= f <= 0.0  # minus the sum of three smoothed AUCs
    assert np.array_equal(np.diag(K), np.ones(len(labels))) and not np.any(G[0])
