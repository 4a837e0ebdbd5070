"""Feature sets and the host path of the feature-vector Grams
(csrc/host/feature_gram.cpp) against the reference's own read_data, dot and
calculate_matrix (tests/golden/feature_gram.json and .npz, from a harness that includes
optimizer/{rbf,poly,sigmoid}_kernel.cpp in place), bit for bit: the dot is
libsvm's sparse merge, the epilogue the reference's operations in its order,
and exp / tanh / cosh are the same libm's."""
import io
import re

import numpy as np
import pytest

import stem_kernel_amd as ska
from stem_kernel_amd import optimizer
from tests import feature_ref
from tests.feature_ref import same_bits

GOLD = feature_ref.golden()


@pytest.fixture(scope="module")
def fs():
    return ska.FeatureSet.read(feature_ref.FEATURE_FILE)


def test_reader_agrees_with_read_data(fs):
    n, d, nnz = fs.shape
    assert n == GOLD["n"] and list(fs.labels) == GOLD["labels"]
    rp, ix, v = fs.rows()
    got = [[[int(i), float(x).hex()] for i, x in zip(ix[rp[k]:rp[k + 1]], v[rp[k]:rp[k + 1]])] for k in range(n)]
    want = [[[i, float.fromhex(x).hex()] for i, x in row] for row in GOLD["vectors"]]
    assert got == want
    # the cases the fixture is there for
    assert 0 in GOLD["labels"] and [] in GOLD["vectors"]
    assert any(x == 0.0 for row in want for _, x in map(lambda t: (t[0], float.fromhex(t[1])), row))
    assert max(i for row in want for i, _ in row) == 2 ** 31 - 2
    assert d == len({i for row in want for i, _ in row}) and nnz == sum(len(r) for r in want)
    with open(feature_ref.FEATURE_FILE) as f:
        parsed = ska.FeatureSet.parse(f.read())
    assert same_bits(ska.feature_dots(parsed), ska.feature_dots(fs))


@pytest.mark.parametrize("text, line, what", [
    ("1 1:2\n-1 1:1 3\n", 2, "no ':'"),
    ("1 1:2\n\n-1 -1:4\n", 3, "negative"),
    ("1 2:1 2:3\n", 1, "ascending"),
    ("1 1:1\n1 1:1\n1 1:1\n-1 5:1 4:1\n", 4, "ascending"),
    ("1 1:1\n1 1:nan\n", 2, "not finite"),
    ("1 1:inf\n", 1, "not finite"),
    ("1 1:1e999\n", 1, "not finite"),
    ("1 1:2x\n", 1, "not a number"),
    ("1 x:2\n", 1, "not an integer"),
])
def test_reader_rejects_with_the_line(text, line, what):
    with pytest.raises(ska.StemKernelError) as e:
        ska.FeatureSet.parse(text)
    assert e.value.code == -1 and f"line {line}:" in str(e.value) and what in str(e.value)


def test_from_arrays_rejects():
    for rp, ix, v in (([0, 2], [3, 3], [1.0, 1.0]), ([0, 1], [-1], [1.0]), ([0, 1], [1], [np.inf])):
        with pytest.raises(ska.StemKernelError):
            ska.FeatureSet.from_arrays(rp, ix, v)


def test_host_dots_and_poly_equal_the_reference_bit_for_bit(fs):
    assert same_bits(ska.feature_dots(fs), GOLD["D"])
    polys = [c for c in GOLD["cases"] if isinstance(c["kernel"], ska.PolyKernel)]
    assert {c["kernel"].degree for c in polys} == {1, 4}
    for c in polys:
        K, G = ska.feature_gram(fs, c["kernel"])
        assert same_bits(K, c["K"]) and same_bits(G, c["G"]), c["name"]
    t = polys[1]["kernel"].gamma * GOLD["D"] + polys[1]["kernel"].coef0
    assert t.min() < 0 < t.max()  # the even degree sees negative bases


def test_host_rbf_and_sigmoid_equal_the_reference_bit_for_bit(fs):
    rest = [c for c in GOLD["cases"] if not isinstance(c["kernel"], ska.PolyKernel)]
    assert len(rest) == 4
    for c in rest:
        K, G = ska.feature_gram(fs, c["kernel"], n_threads=3)
        assert same_bits(K, c["K"]), c["name"]
        assert same_bits(G, c["G"]), c["name"]


def test_column_compaction_changes_nothing():
    a, X = feature_ref.random_set(37, 29, 0xF00D, density=0.6, empty_rows=(4,))
    rp, ix, v = a.rows()
    far = np.linspace(0, 2 ** 31 - 2, 29).astype(np.int64)  # order-preserving, up to 2^31 - 2
    b = ska.FeatureSet.from_arrays(rp, far[ix - 1], v, a.labels)
    assert b.shape == a.shape and int(b.rows()[1].max()) == 2 ** 31 - 2
    assert same_bits(ska.feature_dots(a), ska.feature_dots(b))
    # and the dense in-order sum is the sparse merge: numpy's own loop over the shared columns
    D = ska.feature_dots(a)
    for i, j in ((0, 1), (3, 4), (7, 7), (36, 2)):
        s = 0.0
        for k in range(29):
            if X[i, k] != 0 and X[j, k] != 0:
                s += X[i, k] * X[j, k]
        assert D[i, j] == s
    for kern in feature_ref.kernels():
        Ka, Ga = ska.feature_gram(a, kern)
        Kb, Gb = ska.feature_gram(b, kern)
        assert same_bits(Ka, Kb) and same_bits(Ga, Gb), kern
        assert same_bits(ska.feature_gram_cross(a, a, kern), ska.feature_gram_cross(b, b, kern))


def test_exactly_symmetric_and_rbf_diagonal(fs):
    for kern in feature_ref.kernels():
        K, G = ska.feature_gram(fs, kern)
        assert same_bits(K, K.T) and all(same_bits(g, g.T) for g in G), kern
        if isinstance(kern, ska.RBFKernel):
            assert np.all(np.diag(K) == 1.0)
            assert np.all(np.diag(G[0]) == 0.0) and np.all(np.signbit(np.diag(G[0])))  # -w e with w = +0


def test_cross_of_a_set_with_itself_is_the_symmetric_gram(fs):
    other, _ = feature_ref.random_set(9, 12, 0xBEEF, density=0.5)
    for kern in feature_ref.kernels():
        K, _ = ska.feature_gram(fs, kern)
        assert same_bits(ska.feature_gram_cross(fs, fs, kern), K), kern
        # a rectangular call over the union of both sets' columns: rows of the joint Gram
        R = ska.feature_gram_cross(other, fs, kern)
        assert R.shape == (9, len(fs))
        rp1, ix1, v1 = other.rows()
        rp2, ix2, v2 = fs.rows()
        both = ska.FeatureSet.from_arrays(np.concatenate([rp1, rp1[-1] + rp2[1:]]), np.concatenate([ix1, ix2]),
                                          np.concatenate([v1, v2]))
        assert same_bits(R, ska.feature_gram(both, kern)[0][:9, 9:]), kern
    assert same_bits(ska.feature_dots(other, fs), ska.feature_dots(fs, other).T)


def test_limits_are_reported_and_enforced_on_the_host():
    sh = ska.feature_gram_shape()
    assert sh["tile"] >= 16 and sh["k_slice"] >= 2 and sh["max_n"] >= 4096 and sh["max_dense"] >= sh["max_n"] * 1024
    n = sh["max_n"] + 1
    big = ska.FeatureSet.from_arrays(np.arange(n + 1), np.ones(n, dtype=np.int32), np.ones(n))
    with pytest.raises(ska.StemKernelError) as e:
        ska.feature_gram(big, ska.RBFKernel())
    assert e.value.code == -6 and "max_n" in str(e.value)


def test_cli_defaults_are_the_reference_clis():
    a = optimizer.parser().parse_args(["poly", "x"])
    assert (a.degree, a.gamma, a.coef0, a.cost, a.epsilon, a.factr, a.pgtol, a.nfold) == \
        (3, 1.0, 0.0, 1.0, 0.001, 1e10, 1e-5, 10)
    a = optimizer.parser().parse_args("sigmoid -g 2 -r -1 -c 4 -e 0.01 -v 5 --factr 1e7 --pgtol 1e-3 x".split())
    assert (a.gamma, a.coef0, a.cost, a.epsilon, a.nfold, a.factr, a.pgtol) == (2.0, -1.0, 4.0, 0.01, 5, 1e7, 1e-3)
    k = ska.PolyKernel()
    assert (k.degree, k.gamma, k.coef0) == (3, 1.0, 0.0)
    assert ska.RBFKernel().gamma == 1.0 and (ska.SigmoidKernel().gamma, ska.SigmoidKernel().coef0) == (1.0, 0.0)
    assert ska.SigmoidKernel().bounds == [(1e-5, None), (None, None)]


def test_cli_step_is_the_host_composition(tmp_path, capsys):
    fs40, X = feature_ref.random_set(40, 6, 0xC11, density=0.8)
    path = tmp_path / "train.txt"
    path.write_text("".join(f"{'+1' if y > 0 else '-1'} " + " ".join(f"{k + 1}:{float(x)!r}" for k, x in enumerate(row) if x)
                            + "\n" for y, row in zip(fs40.labels, X)))
    assert optimizer.main(["sigmoid", "--host", "-g", "0.05", "-r", "0.1", "-c", "2", "-v", "5", "--max-steps", "1",
                           str(path)]) == 0
    out = capsys.readouterr().out
    step = out.split("=== Step 1 ===")[1].split("=== Step")[0]
    x = [float(v) for v in re.search(r" x=\[ (.*?)\]", step).group(1).split()]
    f = float(re.search(r" f= (\S+)", step).group(1))
    g = [float(v) for v in re.search(r" g=\[ (.*?)\]", step).group(1).split()]
    assert x == [2.0, 0.05, 0.1] and "....." in step and "Optimized Parameters:" in out
    f0, g0, _ = ska.feature_auc_objective(ska.FeatureSet.read(str(path)), ska.SigmoidKernel(0.05, 0.1), 5, 2.0)
    assert f == float(f"{-f0:.6g}") and g == [float(f"{-v:.6g}") for v in g0]
    buf = io.StringIO()
    optimizer.print_step(3, [1.0, 0.5], -0.75, [0.25, -2.0], out=buf, n_folds=2)
    assert buf.getvalue() == ("=== Step 3 ===\n- calculate a kernel matrix done.\n- gradient calculation \n"
                              " x=[ 1 0.5 ]\n  .. done.\n f= 0.75\n g=[ -0.25 2 ]\n\n")
