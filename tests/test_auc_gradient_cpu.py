"""The optimizer's cross-validated AUC gradient on the host path
(sk_auc_gradient_batch_host, sk_auc_delta; csrc/host/auc_gradient.cpp) against
the reference's own stage functions (tests/golden/auc_gradient.json, made by
tools/make_golden_auc_gradient.py from optimizer/gradient.cpp compiled over
the Boost stand-ins): bit for bit, because the conjugate gradient on the
indefinite KKT system amplifies rounding and no tolerance can be named."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from tests import auc_ref
from tests.auc_ref import as_problem, bits, hexes

PROBLEMS, MATS = auc_ref.fixture()
NAMES = [p["name"] for p in PROBLEMS]


def host(p, **kw):
    K, G, y = auc_ref.inputs(p, MATS)
    return ska.auc_gradient_batch(K, G, y, [as_problem(p)], **kw)[0]


def test_fixture_covers_the_cases():
    by = {p["name"]: p for p in PROBLEMS}
    assert sum(p["natural"] for p in PROBLEMS) == 20
    assert [by[f"crafted n_free={k}"]["n_free"] for k in (0, 1, 2, 10)] == [0, 1, 2, 10]
    assert by["crafted all at the bound"]["n_bound"] == len(by["crafted all at the bound"]["train"])
    assert by["n_params = 0"]["g"] == [] and all(len(p["g"]) == 3 for p in PROBLEMS if p["k"] == 0 and p["g"])
    assert by["permuted training list"]["train"] != sorted(by["permuted training list"]["train"])
    K = MATS[by["non-symmetric K"]["k"]][0]
    assert not np.array_equal(K, K.T)
    y = MATS[0][1]
    assert {y[t] > 0 for t in by["one-class test list"]["test"]} == {True}
    # both ends of the conjugate gradient: the early return and more passes than free examples
    assert any(p["n_free"] > 0 and p["cg_iterations"] == 0 for p in PROBLEMS)
    assert any(p["cg_iterations"] > p["n_free"] > 0 for p in PROBLEMS)


@pytest.mark.parametrize("name", NAMES)
def test_host_path_is_the_reference_bit_for_bit(name):
    p = PROBLEMS[NAMES.index(name)]
    r = host(p, n_threads=1)
    assert (r.n_free, r.n_bound, r.cg_iterations) == (p["n_free"], p["n_bound"], p["cg_iterations"])
    assert r.finite
    assert np.array_equal(bits(r.d_u), bits(hexes(p["d_u"])))
    assert bits([r.cg])[0] == bits([float.fromhex(p["cg"])])[0]
    assert len(r.fg) == len(p["g"]) and np.array_equal(bits(r.fg), bits(hexes(p["fg"])))


def test_one_class_test_list_gives_zero():
    p = next(p for p in PROBLEMS if p["name"] == "one-class test list")
    y = MATS[p["k"]][1]
    f, delta = ska.auc_delta(hexes(p["dec"]), y[p["test"]])
    assert f == 0.0 and not delta.any() and float.fromhex(p["f"]) == 0.0
    r = host(p)
    assert r.cg == 0.0 and not r.fg.any() and not r.d_u.any() and r.cg_iterations == 0 and r.n_free == 6


def test_batch_is_its_problems():
    """Problems over one Gram in one call on several threads, and reversed."""
    ps = [p for p in PROBLEMS if p["k"] == 0 and len(p["g"]) == 3]
    K, G, y = auc_ref.inputs(ps[0], MATS)
    for order in (ps, ps[::-1]):
        for p, r in zip(order, ska.auc_gradient_batch(K, G, y, [as_problem(p) for p in order], n_threads=4)):
            assert np.array_equal(bits(r.d_u), bits(hexes(p["d_u"]))), p["name"]
            assert np.array_equal(bits(r.fg), bits(hexes(p["fg"]))), p["name"]


def test_auc_delta_against_the_fixture():
    """f and delta within (m + 8) 2^-53 sum |term|: m sequential adds and a
    few ulp of exp per term.  Zero where the libm is the fixture's."""
    worst = 0.0
    for p in PROBLEMS:
        y = MATS[p["k"]][1][p["test"]]
        dec = hexes(p["dec"])
        f, delta = ska.auc_delta(dec, y)
        pos, neg = np.flatnonzero(y >= 0), np.flatnonzero(y < 0)
        m = len(pos) * len(neg)
        if m == 0:
            assert f == 0.0 and not delta.any()
            continue
        # the terms, recomputed plainly: sig / m for f, |w| per pair for delta
        d = (dec[pos][:, None] - dec[neg][None, :])
        var = max(float((d * d).mean() - d.mean() ** 2), 1e-10)
        s = 10.0 / np.sqrt(var)
        s2 = -10.0 / (m * np.sqrt(var) * var)
        sig = 1.0 / (1.0 + np.exp(-s * d))
        w = np.abs(sig * (1.0 - sig) * (s + d * s2 * (d - d.mean())) / m)
        unit = (m + 8) * 2.0 ** -53
        assert abs(f - float.fromhex(p["f"])) <= unit * float((sig / m).sum()), p["name"]
        bound = np.zeros(len(dec))
        bound[pos] += w.sum(axis=1)
        bound[neg] += w.sum(axis=0)
        diff = np.abs(delta - hexes(p["delta"]))
        assert np.all(diff <= unit * bound), (p["name"], diff.max())
        worst = max(worst, float(diff.max()), abs(f - float.fromhex(p["f"])))
    print(f"\nauc_delta: largest difference from the fixture {worst:.3g}")


def test_shrinking_record():
    """compute() trains with shrinking = 1 (gradient.cpp:224); the engine
    trains without.  Printed, not asserted: the spread is the reference's own
    noise."""
    print()
    for p in PROBLEMS:
        if not p["natural"]:
            continue
        s = p["shrink"]
        rel = lambda a, b: abs(float.fromhex(a) - float.fromhex(b)) / max(abs(float.fromhex(a)), 1e-300)
        print(f"{p['name']:24s} n_free={p['n_free']:3d} engine cg={float.fromhex(p['cg']): .6e} "
              f"compute() cg={float.fromhex(s['cg']): .6e}  rel f {rel(p['f'], s['f']):.1e} cg {rel(p['cg'], s['cg']):.1e} fg "
              + " ".join(f"{rel(a, b):.1e}" for a, b in zip(p["fg"], s["fg"])))


@pytest.mark.parametrize("C", [1.0, 64.0])
def test_objective_is_the_folds_summed(C):
    """auc_objective on the host path: the whole chain (training without
    shrinking, decision values, delta, gradient) gives the fixture's per-fold
    values, summed as optimizer.cpp:60-77 does."""
    ps = [p for p in PROBLEMS if p["name"].startswith(f"rbf C={C:g} ")]
    assert len(ps) == 5
    K, G, y = auc_ref.inputs(ps[0], MATS)
    f, g, rec = ska.auc_objective(K, G, y, 5, C)
    wf, wg = 0.0, np.zeros(2)
    for p in ps:
        wf -= float.fromhex(p["f"])
        wg[0] -= float.fromhex(p["cg"])
        wg[1] -= float.fromhex(p["fg"][0])
    for p, r in zip(ps, rec):
        assert np.array_equal(bits(r["solution"].alpha), bits(hexes(p["alpha"]))), p["name"]
        assert np.array_equal(bits(r["solution"].decision), bits(hexes(p["dec"]))), p["name"]
    assert bits([f])[0] == bits([wf])[0] and np.array_equal(bits(g), bits(wg))


def test_optimize_smoke():
    """L-BFGS-B over (C, gamma) on the RBF points: returns, finite, and no
    worse than where it started.  No convergence claim: the gradient is noisy
    by construction."""
    from tests import svm_ref
    r = svm_ref.splitmix64_stream(0x5A17A104, 80)
    pts = np.array([[(int(r[2 * k]) % 2001) / 500.0 - 2.0, (int(r[2 * k + 1]) % 2001) / 500.0 - 2.0]
                    for k in range(40)])
    D = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
    y = MATS[4][1]
    seen = []

    def objective(x):
        K = np.exp(-x[1] * D)
        f, g, _ = ska.auc_objective(K, np.stack([-D * K]), y, 5, x[0])
        seen.append(f)
        return f, g

    res = ska.optimize(objective, [1.0, 0.5], bounds=[(None, 1e3), (1e-3, 10.0)], maxiter=5)
    assert np.all(np.isfinite(res.x)) and np.isfinite(res.fun) and res.x[0] >= 1e-5
    assert res.fun <= seen[0] and len(seen) >= 2


def bad_problems():
    p = PROBLEMS[NAMES.index("crafted n_free=2")]
    q = as_problem(p)
    a, d = q["alpha"], q["delta"]

    def alt(**kw):
        return dict(q, **kw)

    def at(v, k, x):
        v = v.copy()
        v[k] = x
        return v

    return p, {
        "train index = n": alt(train=at(np.array(q["train"]), 0, 300)),
        "train index < 0": alt(train=at(np.array(q["train"]), 0, -1)),
        "test index = n": alt(test=at(np.array(q["test"]), 3, 300)),
        "test index < 0": alt(test=at(np.array(q["test"]), 3, -1)),
        "C = 0": alt(C=0.0),
        "C < 0": alt(C=-1.0),
        "n_test = 0": alt(test=[], delta=[]),
        "n_train = 1": alt(train=q["train"][:1], alpha=a[:1]),
        "alpha is NaN": alt(alpha=at(a, 5, np.nan)),
        "alpha is inf": alt(alpha=at(a, 5, np.inf)),
        "delta is NaN": alt(delta=at(d, 2, np.nan)),
        "delta is -inf": alt(delta=at(d, 2, -np.inf)),
    }


def test_argument_errors():
    p, bad = bad_problems()
    K, G, y = auc_ref.inputs(p, MATS)
    ska.auc_gradient_batch(K, G, y, [as_problem(p)])
    for name, q in bad.items():
        with pytest.raises(ska.StemKernelError) as e:
            ska.auc_gradient_batch(K, G, y, [as_problem(p), q])
        assert e.value.code == -1, name
    # a label 0 among a problem's examples: training would call it negative, sign() positive
    for where in (p["train"][7], p["test"][1]):
        y0 = y.copy()
        y0[where] = 0.0
        with pytest.raises(ska.StemKernelError) as e:
            ska.auc_gradient_batch(K, G, y0, [as_problem(p)])
        assert e.value.code == -1
    # n_params < 0 (below the Python layer, which takes n_params from G's shape)
    import ctypes as C
    from stem_kernel_amd import _lib
    arr = (_lib.AucProblem * 1)()
    info = (_lib.AucInfo * 1)()
    out = np.zeros(4)
    f64 = lambda v: v.ctypes.data_as(_lib._F64P)
    assert ska.lib().sk_auc_gradient_batch_host(f64(K), f64(G), -1, len(y), f64(y), arr, 0, 1, f64(out), f64(out),
                                                None, info) == -1
    # n_params = 0 is allowed: cg alone
    r = ska.auc_gradient_batch(K, None, y, [as_problem(p)])[0]
    assert len(r.fg) == 0 and bits([r.cg])[0] == bits([float.fromhex(p["cg"])])[0]
