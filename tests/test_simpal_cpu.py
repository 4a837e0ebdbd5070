"""Simple palindrome kernel (the reference's simpal tool, simpal/simpal.cpp),
host side: the fixture tests/golden/simpal.json against the reference's own
code, the restatement tests/simpal_ref.py against the fixture, the library's
example builder against the restatement, the dataset rules, export/import and
the drop-in.  No GPU."""
import importlib.util
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import stem_kernel_amd as ska
from stem_kernel_amd import _lib
from tests import simpal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout absent")
U = 2.0 ** -24  # float32 unit roundoff
INVALID, UNSUPPORTED = -1, -6  # SK_ERR_INVALID, SK_ERR_UNSUPPORTED


def load_fixture():
    with open(os.path.join(ROOT, "tests", "golden", "simpal.json")) as f:
        fx = json.load(f)
    for e in fx["examples"]:
        e["bpp"] = np.array(e["bpp"], dtype=np.float64)
        e["dist"] = np.array(e["dist"], dtype=np.int32)
        e["weight"] = np.array([float.fromhex(w) for w in e["weight"]], dtype=np.float32)
    for q in fx["queries"]:
        q["K"] = float.fromhex(q["K"])
    return fx


def restated(e):
    return simpal_ref.entries(e["seq"], e["bpp"], e["seed_length"], e["min_loop"], e["max_dist"])


@pytest.fixture(scope="module")
def fixture():
    fx = load_fixture()
    fx["restated"] = [restated(e) for e in fx["examples"]]
    return fx


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_simpal",
                                                  os.path.join(ROOT, "tools", "make_golden_simpal.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bits(w):
    return np.asarray(w, np.float32).view(np.uint32)


@needs_ref
def test_fixture_is_the_references_output_bit_for_bit(tmp_path):
    gen = _generator()
    exe = gen.build_harness(REF, str(tmp_path))
    with open(os.path.join(ROOT, "tests", "golden", "simpal.json")) as f:
        fx = json.load(f)
    ex = gen.examples()
    qs = gen.queries(ex)
    given = ("group", "set", "seq", "seed_length", "min_loop", "max_dist", "bpp", "n_max")
    assert [{k: e[k] for k in given} for e in fx["examples"]] == ex
    assert [{k: q[k] for k in ("x", "y", "tolerance")} for q in fx["queries"]] == qs
    ents, vals = gen.reference_output(exe, str(tmp_path), ex, qs)
    assert [(e["keys"], e["dist"], e["weight"]) for e in fx["examples"]] == ents
    assert [q["K"] for q in fx["queries"]] == vals


def test_fixture_holds_the_cases(fixture):
    ex = fixture["examples"]
    exact = [e for e in ex if e["group"] == "exact"]
    ordered = [e for e in ex if e["group"] == "ordered"]
    assert all(e["n_max"] <= 2 for e in exact) and all(e["n_max"] >= 3 for e in ordered) and ordered
    assert {3, 4, 7, 21, 60, 100} <= {len(e["seq"]) for e in exact}
    assert any(len(e["keys"]) == 0 and len(e["seq"]) > 10 for e in exact)  # no palindrome
    assert any("t" in e["seq"] and "n" in e["seq"] and any(c.isupper() for c in e["seq"]) and len(e["keys"])
               for e in exact)
    assert {e["seed_length"] for e in exact} == {1, 3, 5}
    assert {e["min_loop"] for e in exact} == {0, 3}
    cut = [e for e in exact if e["max_dist"] < 300]
    assert cut and all(len(simpal_ref.entries(e["seq"], e["bpp"], e["seed_length"], e["min_loop"], 300)[0])
                       > len(e["keys"]) for e in cut)
    for e in ex:
        tols = {q["tolerance"] for q in fixture["queries"] if q["x"] == fixture["examples"].index(e)}
        assert tols == {-1, 0, 1, e["seed_length"]}
    assert any(q["K"] > 0 for q in fixture["queries"])


def test_restatement_equals_the_reference(fixture):
    """exact group: bit for bit, entries and K.  ordered group: two float
    orderings of n non-negative terms each lie within (n - 1) 2^-24 of the
    true sum, so entries agree within 2 (n_max - 1) 2^-24; K is bilinear in
    the weights, hence 4 (n_max - 1) 2^-24 (relative)."""
    ex = fixture["examples"]
    for e, (k, d, w) in zip(ex, fixture["restated"]):
        assert k == e["keys"] and np.array_equal(d, e["dist"])
        if e["group"] == "exact":
            assert np.array_equal(_bits(w), _bits(e["weight"]))
        else:
            bound = 2 * (e["n_max"] - 1) * U
            assert np.all(np.abs(w.astype(np.float64) - e["weight"]) <= bound * e["weight"].astype(np.float64))
    worst = 0.0
    for q in fixture["queries"]:
        got = simpal_ref.kernel_seq(fixture["restated"][q["x"]], fixture["restated"][q["y"]], q["tolerance"])
        if ex[q["x"]]["group"] == "exact":
            assert got == q["K"], q
        else:
            n_max = max(ex[q["x"]]["n_max"], ex[q["y"]]["n_max"])
            assert abs(got - q["K"]) <= 4 * (n_max - 1) * U * q["K"], q
            worst = max(worst, abs(got - q["K"]) / q["K"] if q["K"] else 0.0)
    print(f"ordered group: worst relative deviation of K {worst:.3g}")


def test_library_builder_equals_the_restatement(fixture):
    """add_palindromes -> palindromes(i): the same defined order of the float
    sums, so bit for bit on every fixture example of both groups."""
    for e, (k, d, w) in zip(fixture["examples"], fixture["restated"]):
        ds = ska.Dataset()
        ds.add_palindromes("+1", e["seq"], e["bpp"], e["seed_length"], e["min_loop"], e["max_dist"])
        gk, gd, gw = ds.palindromes(0)
        assert gk == k and np.array_equal(gd, d) and np.array_equal(_bits(gw), _bits(w)), e["seq"]


def test_vectorised_restatement_equals_the_sequential(fixture):
    for q in fixture["queries"]:
        a, b = fixture["restated"][q["x"]], fixture["restated"][q["y"]]
        s, v = simpal_ref.kernel_seq(a, b, q["tolerance"]), simpal_ref.kernel_vec(a, b, q["tolerance"])
        assert abs(s - v) <= 1e-12 * abs(s)


def _code(e):
    return e.value.code


def test_refusals():
    bpp = lambda n: np.zeros(n * (n - 1) // 2)
    ds = ska.Dataset()
    with pytest.raises(ska.StemKernelError) as e:  # n < seed_length: the reference's loop bound wraps
        ds.add_palindromes("+1", "ac", bpp(2), seed_length=3)
    assert _code(e) == INVALID
    for s in (0, 33):
        with pytest.raises(ska.StemKernelError) as e:
            ds.add_palindromes("+1", "acgu" * 10, bpp(40), seed_length=s)
        assert _code(e) == UNSUPPORTED
        with pytest.raises(ska.StemKernelError) as e:
            ds.add_palindrome_entries("+1", [], [], [], seed_length=s)
        assert _code(e) == UNSUPPORTED
    assert len(ds) == 0
    ds.add_palindromes("+1", "acguacgu", bpp(8), seed_length=3)
    with pytest.raises(ska.StemKernelError) as e:  # one seed_length per dataset
        ds.add_palindromes("+1", "acguacgu", bpp(8), seed_length=2)
    assert _code(e) == INVALID
    with pytest.raises(ska.StemKernelError) as e:
        ds.add_palindrome_entries("+1", ["ac"], [3], [1.0])
    assert _code(e) == INVALID
    # a dataset is of one sort
    with pytest.raises(ska.StemKernelError) as e:
        ds.add("+1", ["ACGU"], use_bp=False)
    assert _code(e) == INVALID
    with pytest.raises(ska.StemKernelError) as e:
        ds.add_protein("+1", ["MKV"])
    assert _code(e) == INVALID
    for other in ("rna", "protein"):
        o = ska.Dataset()
        if other == "rna":
            o.add("+1", ["ACGU"], use_bp=False)
        else:
            o.add_protein("+1", ["MKV"])
        with pytest.raises(ska.StemKernelError) as e:
            o.add_palindromes("+1", "acguacgu", bpp(8))
        assert _code(e) == INVALID
        with pytest.raises(ska.StemKernelError) as e:
            o.add_palindrome_entries("+1", ["acg"], [3], [1.0])
        assert _code(e) == INVALID
        with pytest.raises(ska.StemKernelError):
            o.palindromes(0)
        c = ska.Dataset()
        c.add_palindrome_entries("+1", ["acg"], [3], [1.0])
        assert lib_add_copy(c, o, 0) == INVALID
    assert len(ds) == 1
    two = ska.Dataset()
    two.add_palindrome_entries("+1", ["ac"], [3], [1.0])
    assert lib_add_copy(ds, two, 0) == INVALID  # another seed_length


def lib_add_copy(dst, src, i):
    return ska.lib().sk_dataset_add_copy(dst.handle, src.handle, i)


@pytest.mark.parametrize("keys,dist,weight", [
    (["acg", "acn"], [1, 2], [1.0, 1.0]),        # a letter outside acgu
    (["acg", "ACG"], [1, 2], [1.0, 1.0]),        # uppercase
    (["acg", "acu"], [1, -2], [1.0, 1.0]),       # negative dist
    (["acg", "acu"], [1, 2], [1.0, -0.5]),       # negative weight
    (["acg", "acu"], [1, 2], [1.0, np.inf]),     # not finite
    (["acg", "acu"], [1, 2], [np.nan, 1.0]),
    (["acg", "acu", "acg"], [1, 2, 1], [1.0, 1.0, 2.0]),  # a duplicate (key, dist)
])
def test_entries_that_are_refused(keys, dist, weight):
    ds = ska.Dataset()
    with pytest.raises(ska.StemKernelError) as e:
        ds.add_palindrome_entries("+1", keys, dist, weight)
    assert _code(e) == INVALID and len(ds) == 0


def test_entries_round_trip_sorted():
    ds = ska.Dataset()
    keys = ["uuu", "acg", "acg", "aaa", "gca", "acg"]
    dist = [4, 9, 2, 7, 0, 2 ** 30]
    w = np.array([0.5, 0.25, 1.5, 0.0, 3.0e-7, 2.0], np.float32)
    ds.add_palindrome_entries("x", keys, dist, w)
    ds.add_palindrome_entries("y", [], [], [], seed_length=3)
    k, d, g = ds.palindromes(0)
    order = sorted(range(6), key=lambda i: (keys[i], dist[i]))
    assert k == [keys[i] for i in order] == ["aaa", "acg", "acg", "acg", "gca", "uuu"]
    assert list(d) == [dist[i] for i in order] and np.array_equal(_bits(g), _bits(w[order]))
    assert ds.palindromes(1)[0] == [] and ds.label(0) == "x" and len(ds) == 2
    # 32 letters fill the key word
    ds32 = ska.Dataset()
    k32 = ["u" * 32, "a" * 32, "acgu" * 8, "u" * 31 + "g"]
    ds32.add_palindrome_entries("+1", k32, [1, 1, 1, 1], [1, 2, 3, 4])
    assert ds32.palindromes(0)[0] == sorted(k32)


def _pal_dataset(fixture, set_="s3"):
    ds = ska.Dataset()
    for e in fixture["examples"]:
        if e["set"] == set_:
            ds.add_palindromes(e["seq"][:4], e["seq"], e["bpp"], e["seed_length"], e["min_loop"], e["max_dist"])
    return ds


def test_export_import_round_trip(fixture):
    ds = _pal_dataset(fixture)
    n = len(ds)
    blob = ds.export()
    assert struct.unpack_from("<III", blob) == (0x58454B53, 3, n)
    back = ska.Dataset().import_bytes(blob)
    assert len(back) == n and back.pack_digest() == ds.pack_digest()
    for i in range(n):
        a, b = ds.palindromes(i), back.palindromes(i)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[2]), _bits(b[2]))
        assert back.label(i) == ds.label(i)
    # a share of the examples, then the rest: the whole again
    parts = ska.Dataset().import_bytes(ds.export(0, 4)).import_bytes(ds.export(4))
    assert parts.pack_digest() == ds.pack_digest() and parts.export() == blob
    # add_copy carries the sort
    c = ska.Dataset()
    assert lib_add_copy(c, ds, 5) == 0
    assert c.palindromes(0)[0] == ds.palindromes(5)[0]
    # into a dataset of another sort or seed_length: refused, nothing appended
    rna = ska.Dataset()
    rna.add("+1", ["ACGU"], use_bp=False)
    two = ska.Dataset()
    two.add_palindrome_entries("+1", ["ac"], [3], [1.0])
    for other in (rna, two):
        with pytest.raises(ska.StemKernelError):
            other.import_bytes(blob)
        assert len(other) == 1


def test_corrupted_buffer_is_rejected():
    ds = ska.Dataset()
    ds.add_palindrome_entries("+1", ["aca", "acg", "gcu"], [5, 6, 7], [0.5, 0.25, 0.125])
    blob = bytes(ds.export())
    assert len(ska.Dataset().import_bytes(blob)) == 1
    m = 3
    w0 = len(blob) - 4 * m        # the weights end the buffer; before them their count,
    d0 = w0 - 8 - 4 * m           # the dists, their count,
    k0 = d0 - 8 - 8 * m           # and the keys
    assert struct.unpack_from("<3f", blob, w0) == (0.5, 0.25, 0.125)
    assert struct.unpack_from("<3i", blob, d0) == (5, 6, 7)
    keys = struct.unpack_from("<3Q", blob, k0)
    assert keys == (0b000100, 0b000110, 0b100111)

    def patched(*edits):
        b = bytearray(blob)
        for off, fmt, v in edits:
            struct.pack_into(fmt, b, off, *v)
        return bytes(b)

    bad = [
        patched((w0 + 4, "<f", [float("nan")])),
        patched((w0, "<f", [float("inf")])),
        patched((w0 + 8, "<f", [-1.0])),
        patched((d0 + 4, "<i", [-6])),
        patched((k0, "<2Q", [keys[1], keys[0]])),                         # not in map order
        patched((k0, "<2Q", [keys[1], keys[1]]), (d0, "<2i", [6, 6])),    # a duplicate (key, dist)
        patched((k0 + 8, "<Q", [keys[1] | (1 << 6)])),                    # a letter past seed_length
        patched((k0 - 8 - 4, "<i", [0])),                                 # seed_length 0
        patched((k0 - 8 - 4, "<i", [33])),
        blob[:-1],
        blob + b"\0",
        patched((4, "<I", [4])),                                          # an unknown version
    ]
    for k, b in enumerate(bad):
        t = ska.Dataset()
        with pytest.raises(ska.StemKernelError):
            t.import_bytes(b)
        assert len(t) == 0, k


def test_rna_and_protein_exports_keep_their_bytes():
    """Version 3 is written only when the range holds a palindrome example."""
    rna = ska.Dataset()
    rna.add("+1", ["ACGUACGUAC"], use_bp=False)
    prot = ska.Dataset()
    prot.add_protein("+1", ["MKVLA"])
    assert struct.unpack_from("<II", rna.export()) == (0x58454B53, 1)
    assert struct.unpack_from("<II", prot.export()) == (0x58454B53, 2)
    # byte for byte what the fields of versions 1 and 2 are: the label, then
    # the example's fields, no palindrome fields after them
    b = bytes(prot.export())
    assert b.endswith(struct.pack("<BQ", 1, 5 * 24) + prot.aa_profile(0)[0].tobytes())
    r = bytes(rna.export())
    assert ska.Dataset().import_bytes(r).export() == r and ska.Dataset().import_bytes(b).export() == b


def test_symbols_enum_and_defaults():
    L = ska.lib()
    for name in ("sk_dataset_add_palindromes", "sk_dataset_add_palindromes_folded",
                 "sk_dataset_add_palindrome_entries", "sk_dataset_palindromes", "sk_simpal_shape"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert _lib.SIMPAL == 16
    p = ska.SimpalKernel().params
    assert p.kind == 16 and p.mismatch == 1.0
    assert ska.SimpalKernel(tolerance=-1).params.mismatch == -1.0
    assert ska.default_params(_lib.SIMPAL).mismatch == 1.0
    assert ska.default_params(_lib.SI_STR).mismatch == 0.8  # the other kinds keep theirs
    with pytest.raises(ValueError):
        ska.SimpalKernel(tolerance=0.5)
    t, b = ska.simpal_shape()
    assert t >= 64 and b >= 1
    # two workgroups' tiles fit a CU's 160 KB of LDS (20 B per y entry, 748 table doubles)
    assert 2 * (t * 20 + 748 * 8) <= 160 * 1024
    with open(os.path.join(ROOT, "include", "stem_kernel.h")) as f:
        text = f.read()
    assert "SK_SIMPAL = 16" in text and "#define SK_ABI_VERSION 3" in text


def build_dropin(tmp_path, name="simpal_dropin"):
    libdir = os.path.join(ROOT, "stem_kernel_amd")
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-L", libdir, "-lstem_kernel_amd",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    return exe


def test_simpal_dropin_main_compiles(tmp_path):
    """tests/cpp/simpal_dropin.cpp, a main in the shape of simpal.cpp:282-423
    over include/simpal_compat.hpp."""
    assert os.path.exists(build_dropin(tmp_path))
