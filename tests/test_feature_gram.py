"""Feature-vector Grams on the GPU (sk_feature_gram, sk_feature_gram_cross,
sk_feature_dots; csrc/kernels/feature_gram.hip) against the host path
(csrc/host/feature_gram.cpp) and the reference's own values
(tests/golden/feature_gram.json and .npz).  The dot matrix and the whole polynomial
kernel are bit for bit; exp / tanh / cosh are the device library's, so the RBF
and sigmoid kernels meet the project's 1e-6 relative bound (the measured
deviation in ulps is printed, and recorded in DESIGN.md 17).  The shapes are the
smallest that cross every boundary of the dot kernel: its tile edge T and
k-slice S (sk_feature_gram_shape)."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from tests import feature_ref
from tests.feature_ref import rel_close, same_bits, ulps

pytestmark = pytest.mark.gpu
SHAPE = ska.feature_gram_shape()
T, S = SHAPE["tile"], SHAPE["k_slice"]
GOLD = feature_ref.golden()


def _sets():
    """name -> FeatureSet: every n in {1, T-1, T+1, 2T+2} with every d in
    {1, S-1, S+1, 2S+1}, a set with empty rows, and a 5 %-dense one with
    far-apart indices."""
    ns, ds = [1, T - 1, T + 1, 2 * T + 2], [1, S - 1, S + 1, 2 * S + 1]
    out = {}
    for n in ns:
        for d in ds:
            out[f"n={n} d={d}"] = feature_ref.random_set(n, d, 0xFEA7 + 16 * n + d)[0]
    out["empty rows"] = feature_ref.random_set(T + 3, S + 2, 0xFEA8, density=0.5, empty_rows=(0, 5, T + 2))[0]
    out["5 % dense, far apart"] = feature_ref.random_set(2 * T + 2, 300, 0xFEA9, density=0.05, spread=7000001)[0]
    return out


@pytest.fixture(scope="module")
def sets():
    """The sets, and per set the host path's D and (K, G) per kernel, computed once."""
    s = _sets()
    host = {k: dict(D=ska.feature_dots(fs), grams=[ska.feature_gram(fs, kern) for kern in feature_ref.kernels()])
            for k, fs in s.items()}
    return s, host


def test_shape_is_exported():
    assert T >= 16 and S >= 2 and SHAPE["max_n"] >= 4096


def test_dots_equal_the_host_bit_for_bit(gpu_ctx, sets):
    s, host = sets
    for name, fs in s.items():
        assert same_bits(ska.feature_dots(fs, ctx=gpu_ctx), host[name]["D"]), name
    # rectangular, unequal n, columns compacted over the union of both sets
    for a, b in (("n=1 d=1", "n=%d d=%d" % (2 * T + 2, 2 * S + 1)), ("n=%d d=%d" % (T + 1, S + 1), "empty rows"),
                 ("5 % dense, far apart", "n=%d d=%d" % (T - 1, S - 1))):
        got = ska.feature_dots(s[a], s[b], ctx=gpu_ctx)
        assert got.shape == (len(s[a]), len(s[b]))
        assert same_bits(got, ska.feature_dots(s[a], s[b])), (a, b)
    fs = ska.FeatureSet.read(feature_ref.FEATURE_FILE)
    assert same_bits(ska.feature_dots(fs, ctx=gpu_ctx), GOLD["D"])


def test_poly_equals_the_host_bit_for_bit(gpu_ctx, sets):
    s, host = sets
    for name, fs in s.items():
        for kern, (K, G) in zip(feature_ref.kernels(), host[name]["grams"]):
            if isinstance(kern, ska.PolyKernel):
                Kg, Gg = ska.feature_gram(fs, kern, ctx=gpu_ctx)
                assert same_bits(Kg, K) and same_bits(Gg, G), (name, kern)
    fs = ska.FeatureSet.read(feature_ref.FEATURE_FILE)
    for c in GOLD["cases"]:
        if isinstance(c["kernel"], ska.PolyKernel):
            Kg, Gg = ska.feature_gram(fs, c["kernel"], ctx=gpu_ctx)
            assert same_bits(Kg, c["K"]) and same_bits(Gg, c["G"]), c["name"]
    a, b = s["empty rows"], s["n=%d d=%d" % (T - 1, S - 1)]
    kern = ska.PolyKernel(4, 0.05, -1.0)
    assert same_bits(ska.feature_gram_cross(a, b, kern, ctx=gpu_ctx), ska.feature_gram_cross(a, b, kern))


def test_rbf_and_sigmoid_within_the_parity_bound(gpu_ctx, sets):
    s, host = sets
    for name, fs in s.items():
        for kern, (K, G) in zip(feature_ref.kernels(), host[name]["grams"]):
            if isinstance(kern, ska.PolyKernel):
                continue
            Kg, Gg = ska.feature_gram(fs, kern, ctx=gpu_ctx)
            assert same_bits(Kg, Kg.T) and all(same_bits(g, g.T) for g in Gg), (name, kern)
            worst = max([rel_close(Kg, K)] + [rel_close(a, b) for a, b in zip(Gg, G)])
            assert worst <= 1.0, (name, kern, worst)
            if isinstance(kern, ska.RBFKernel):
                assert np.all(np.diag(Kg) == 1.0) and np.all(np.signbit(np.diag(Gg[0])))
    fs = ska.FeatureSet.read(feature_ref.FEATURE_FILE)
    for c in GOLD["cases"]:
        if isinstance(c["kernel"], ska.PolyKernel):
            continue
        Kg, Gg = ska.feature_gram(fs, c["kernel"], ctx=gpu_ctx)
        print(f"ulps against the reference, {c['name']}: K {ulps(Kg, c['K'])}, G "
              + " ".join(str(ulps(a, b)) for a, b in zip(Gg, c["G"])))
        worst = max([rel_close(Kg, c["K"])] + [rel_close(a, b) for a, b in zip(Gg, c["G"])])
        assert worst <= 1.0, (c["name"], worst)
        if isinstance(c["kernel"], ska.RBFKernel):
            a, b = s["empty rows"], fs
            R, Rh = (ska.feature_gram_cross(a, b, c["kernel"], ctx=ctx) for ctx in (gpu_ctx, None))
            assert rel_close(R, Rh) <= 1.0
            assert rel_close(ska.feature_gram_cross(fs, fs, c["kernel"], ctx=gpu_ctx), c["K"]) <= 1.0


def test_dot_matrix_stays_resident(gpu_ctx):
    a = feature_ref.random_set(T + 1, S + 1, 0x7E51)[0]
    b = feature_ref.random_set(T + 1, S + 1, 0x7E52)[0]  # same shape, other values
    k1, k2 = ska.PolyKernel(2, 0.5, 1.0), ska.PolyKernel(3, 0.25, -0.5)
    Ka, Ga = ska.feature_gram(a, k1, ctx=gpu_ctx)
    assert gpu_ctx.last_launch_ms()["launches"] == 2  # feat_dot, feat_apply
    K2, G2 = ska.feature_gram(a, k2, ctx=gpu_ctx)
    assert gpu_ctx.last_launch_ms()["launches"] == 1  # feat_apply alone: D is resident
    Kh, Gh = ska.feature_gram(a, k2)
    assert same_bits(K2, Kh) and same_bits(G2, Gh)
    Kb, Gb = ska.feature_gram(b, k2, ctx=gpu_ctx)
    assert gpu_ctx.last_launch_ms()["launches"] == 2  # a second set has its own D
    Kh, Gh = ska.feature_gram(b, k2)
    assert same_bits(Kb, Kh) and same_bits(Gb, Gh) and not same_bits(Kb, K2)
    assert same_bits(ska.feature_dots(a, ctx=gpu_ctx), ska.feature_dots(a))
    assert gpu_ctx.last_launch_ms()["launches"] == 0
    # a freed set's D goes with it: a new set (whatever its address) is computed afresh
    a.close()
    c = feature_ref.random_set(T + 1, S + 1, 0x7E53)[0]
    Kc, _ = ska.feature_gram(c, k1, ctx=gpu_ctx)
    assert gpu_ctx.last_launch_ms()["launches"] == 2 and same_bits(Kc, ska.feature_gram(c, k1)[0])


@pytest.mark.parametrize("kern", [ska.RBFKernel(0.3), ska.PolyKernel(2, 0.2, 1.0), ska.SigmoidKernel(0.05, 0.1)],
                         ids=["rbf", "poly", "sigmoid"])
def test_objective_is_the_composition(gpu_ctx, kern):
    fs = feature_ref.random_set(40, 6, 0xC0DE, density=0.8)[0]
    K, G = ska.feature_gram(fs, kern, ctx=gpu_ctx)
    f0, g0, _ = ska.auc_objective(K, G, fs.labels, 5, 2.0, ctx=gpu_ctx)
    f, g, rec = gpu_ctx.feature_auc_objective(fs, kern, 5, 2.0)
    assert len(rec) == 5 and len(g) == 1 + len(kern.params)
    assert same_bits([f], [f0]) and same_bits(g, g0)


def test_over_the_limits_is_unsupported_before_any_launch(gpu_ctx):
    n = SHAPE["max_n"] + 1
    big = ska.FeatureSet.from_arrays(np.arange(n + 1), np.ones(n, dtype=np.int32), np.ones(n))
    small = feature_ref.random_set(3, 2, 1)[0]
    for call in (lambda: ska.feature_gram(big, ska.RBFKernel(), ctx=gpu_ctx),
                 lambda: ska.feature_dots(big, ctx=gpu_ctx),
                 lambda: ska.feature_gram_cross(small, big, ska.RBFKernel(), ctx=gpu_ctx)):
        with pytest.raises(ska.StemKernelError) as e:
            call()
        assert e.value.code == -6 and "max_n" in str(e.value)
        assert gpu_ctx.last_launch_ms()["launches"] == 0
    # the dense budget: n x used columns
    n = SHAPE["max_n"]
    d = SHAPE["max_dense"] // n + 1
    rp = np.concatenate([[0], d + np.arange(n)])  # the first example uses d columns, the others one
    wide = ska.FeatureSet.from_arrays(rp, np.concatenate([np.arange(d), np.zeros(n - 1)]), np.ones(d + n - 1))
    assert wide.shape[:2] == (n, d)
    with pytest.raises(ska.StemKernelError) as e:
        ska.feature_gram(wide, ska.PolyKernel(), ctx=gpu_ctx)
    assert e.value.code == -6 and "max_dense" in str(e.value)
    assert gpu_ctx.last_launch_ms()["launches"] == 0
