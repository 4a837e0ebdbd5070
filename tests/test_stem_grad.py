"""Gradients of the DAG stem kernels on the GPU (csrc/kernels/stem_grad.hip):
the GPU call against the host path and the long-double restatement, both
instantiations, batch independence, the composite kinds' values against
Context.pairs and the objective's pass-through.

GPU against the host path, err = |a - b| / (|b| + |K|) per derivative and
|a - b| / |b| for the value, the worst over every unordered pair of the
fixture, the cross-set call and the eight configurations (the tests print
them; MEASURED_WORST holds what the card gave).  The gate is 16 x that worst,
never looser than 1e-9."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from tests import stem_grad_ref as R
from tests import test_stem_grad_cpu as cpu
from tests.helpers import make_examples

pytestmark = pytest.mark.gpu

LONG = 15  # the 150-nt sequence: y levels wider than a wave, rows of several strides
# value 6.53e-15; loop_gap 4.10e-15, beta 3.13e-15, stack 9.8e-16, covar 2.13e-15
MEASURED_WORST = 6.53e-15
GPU_GATE = min(16 * MEASURED_WORST, 1e-9)
NAMES = ("loop_gap", "beta", "stack", "covar")


@pytest.fixture(scope="module")
def data():
    ex = cpu.examples() + [ska.random_sequences(1, 150, 0x150)[0]]
    ds, om = make_examples(ex)
    # the y set of the cross-set call: other examples in another order
    ys_ex = [ex[LONG], ex[12], ex[cpu.EMPTY], ex[3]]
    ys, _ = make_examples(ys_ex)
    return ds, om, ys


def errs(val, grad, hval, hgrad):
    """Worst value error and per-slot derivative error against the host path;
    exact zeros must be exact zeros."""
    zero = hgrad == 0.0
    assert np.array_equal(grad == 0.0, zero) and not np.signbit(grad[zero]).any()
    vz = hval == 0.0
    assert np.array_equal(val == 0.0, vz) and not np.signbit(val[vz]).any()
    ev = np.max(np.abs(val - hval)[~vz] / np.abs(hval[~vz]))
    den = np.abs(hgrad) + np.abs(hval)[:, None]
    eg = np.where(den > 0, np.abs(grad - hgrad) / np.where(den > 0, den, 1.0), 0.0).max(axis=0)
    return ev, eg


def test_against_the_host_path(data, gpu_ctx):
    ds, _, ys = data
    n = len(ds)
    iu, ju = np.triu_indices(n)
    cx, cy = np.meshgrid(np.arange(n), np.arange(len(ys)), indexing="ij")
    cx, cy = cx.ravel(), cy.ravel()
    worst_v, worst_g = 0.0, np.zeros(4)
    ran = set()
    for subst, g, band in cpu.configs():
        kern = cpu.kernel(subst, g, band)
        val, grad = gpu_ctx.stem_gradients(ds, kern, iu, ju)
        assert gpu_ctx.last_launch_ms()["launches"] == 2  # the prep kernel and the pair kernel
        k = ska.stem_grad.stem_last_kernels(gpu_ctx)
        assert k == dict(su=subst, si=not subst)
        ran.add("su" if subst else "si")
        hval, hgrad = ska.stem_gradients(ds, kern, iu, ju)
        ev, eg = errs(val, grad, hval, hgrad)
        e = (iu == cpu.EMPTY) | (ju == cpu.EMPTY)
        assert not val[e].any() and not grad[e].any()
        # ordered pairs across two datasets
        val2, grad2 = gpu_ctx.stem_gradients(ds, kern, cx, cy, ys=ys)
        hval2, hgrad2 = ska.stem_gradients(ds, kern, cx, cy, ys=ys)
        ev2, eg2 = errs(val2, grad2, hval2, hgrad2)
        print(f"subst={subst} loop_gap={g} band={band}: value {max(ev, ev2):.3g}, derivatives",
              dict(zip(NAMES, np.maximum(eg, eg2))))
        worst_v = max(worst_v, ev, ev2)
        worst_g = np.maximum(worst_g, np.maximum(eg, eg2))
    print("GPU against the host path, worst: value", worst_v, "derivatives", dict(zip(NAMES, worst_g)),
          "gate", GPU_GATE)
    assert ran == {"su", "si"}
    assert worst_v <= GPU_GATE and np.all(worst_g <= GPU_GATE)


def test_against_the_long_double_restatement(data, gpu_ctx):
    """The project's 1e-6 gate, on the CPU test's pairs and on the 150-nt
    sequence as x and as y."""
    ds, om, _ = data
    ex = [R.Ex(o) for o in om]
    pairs = list(cpu.REF_PAIRS[:6]) + [(LONG, 0), (1, LONG), (cpu.EMPTY, LONG)]
    px = np.array([i for i, _ in pairs], np.int32)
    py = np.array([j for _, j in pairs], np.int32)
    for subst, g, band in ((True, 0.2, 10), (False, 0.98, 0)):
        kern = cpu.kernel(subst, g, band)
        val, grad = gpu_ctx.stem_gradients(ds, kern, px, py)
        for k, (i, j) in enumerate(pairs):
            r = cpu.ref_pair(ex, subst, kern.params, i, j)
            want = R.row4(subst, r)
            K = float(r[0])
            assert abs(val[k] - K) <= 1e-6 * abs(K), (subst, i, j, val[k], K)
            for s in range(4):
                assert abs(grad[k, s] - float(want[s])) <= 1e-6 * (abs(float(want[s])) + abs(K)), (subst, i, j, s)


def _grid_waves():
    try:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
    except Exception:
        cus = 256
    return cus * 8 * 4  # workgroups per CU x waves per workgroup (host/pairs_stem_grad.cpp)


@pytest.mark.parametrize("subst", [True, False])
def test_a_pair_has_the_same_bits_wherever_it_stands_in_a_batch(data, gpu_ctx, subst):
    """Stale slab or scratch rows would show: the pair runs behind other pairs
    of its wave, costlier and cheaper ones, in three batches of different
    neighbours."""
    ds, _, _ = data
    kern = cpu.kernel(subst, 0.98, 0)
    a, b = 9, 12
    v1, g1 = gpu_ctx.stem_gradients(ds, kern, [a], [b])
    assert v1[0] > 0 and g1[0, 0] > 0
    n = 3 * 4 * _grid_waves()
    small = np.arange(15)  # (not the 150-nt sequence: it would size every wave's scratch)
    for t, pos in enumerate((0, n // 2, n - 1)):
        rng = np.random.default_rng(77 + t)
        x = rng.choice(small, n).astype(np.int32)
        y = rng.choice(small, n).astype(np.int32)
        x[pos], y[pos] = a, b
        val, grad = gpu_ctx.stem_gradients(ds, kern, x, y)
        assert val[pos] == v1[0] and np.array_equal(grad[pos], g1[0]), pos
        # and every copy of a pair in the batch has one set of bits
        key = x.astype(np.int64) * 16 + y
        order = np.argsort(key, kind="stable")
        same = key[order][1:] == key[order][:-1]
        assert np.array_equal(val[order][1:][same], val[order][:-1][same])
        assert np.array_equal(grad[order][1:][same], grad[order][:-1][same])


def test_composite_values_are_context_pairs(data, gpu_ctx):
    ds, _, _ = data
    x = np.array([0, 5, 11, 9, cpu.EMPTY, 3, LONG, 2], np.int32)
    y = np.array([1, 5, 12, 2, 4, cpu.EMPTY, 7, LONG], np.int32)
    v0, g0 = gpu_ctx.stem_gradients(ds, ska.SuStemKernel(), x, y)
    v1, g1 = gpu_ctx.stem_gradients(ds, ska.SiStemKernel(), x, y)
    for kern, gs in ((ska.SuStemStrKernel(), g0), (ska.SiStemStrKernel(), g1), (ska.LSuStemKernel(), None),
                     (ska.LSuStemStrKernel(), None), (ska.SuStemKernel(), g0), (ska.SiStemKernel(), g1)):
        val, grad = gpu_ctx.stem_gradients(ds, kern, x, y)
        want = gpu_ctx.pairs(ds, kern, x, y)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(val), fin) and np.array_equal(val[~fin], want[~fin])
        assert np.all(np.abs(val[fin] - want[fin]) <= 1e-6 * np.abs(want[fin])), type(kern).__name__
        if gs is not None:
            assert np.array_equal(grad, gs)
        else:
            beta = kern.params.beta
            ok = v0 > 0
            assert np.allclose(grad[ok, 0], beta * g0[ok, 0] / v0[ok], rtol=1e-14, atol=0)
            assert np.allclose(grad[ok, 1], np.log(v0[ok]) + beta * g0[ok, 1] / v0[ok], rtol=1e-14, atol=0)
            assert np.isnan(grad[~ok, :2]).all() and not grad[:, 2:].any()
            assert (val[~ok] == -np.inf).all()


def test_auc_objective_is_the_composition_bit_for_bit(gpu_ctx):
    ds, labels = cpu._toy_set()
    bits = lambda a: np.asarray(a, dtype=np.float64).view(np.uint64)  # noqa: E731
    for kern, keep in ((ska.SuStemKernel(), [0, 1, 2]), (ska.SiStemKernel(), [0, 1, 3, 4])):
        f, g, rec = gpu_ctx.stem_auc_objective(ds, kern, labels, 4, 2.0, normalize=True)
        assert np.isfinite(f) and g.shape == (len(keep),) and len(rec) == 4
        K, G = gpu_ctx.stem_gradient_gram(ds, kern, normalize=True)
        f2, g2, _ = ska.auc_objective(K, G, labels, 4, 2.0, ctx=gpu_ctx)
        assert bits([f])[0] == bits([f2])[0]
        g2 = np.asarray(g2)[keep]
        nan = np.isnan(g2)
        assert np.array_equal(np.isnan(g), nan) and np.array_equal(bits(g)[~nan], bits(g2)[~nan])
        assert -4.0 <= f <= 0.0  # minus the sum of four smoothed AUCs
        assert np.array_equal(np.diag(K), np.ones(len(labels)))
