"""Protein local-alignment kernel (the reference's la_kernel,
BPLAKernel<double,AAMData>, bpla_kernel/la_main.cpp:118-135), host side: the
fixture tests/golden/la_protein.json against the reference's own code, the
numpy restatement tests/la_ref.py against the fixture (both bit for bit), the
BLOSUM62 default, the profile, the dataset rules and export/import.  No GPU."""
import ctypes as C
import importlib.util
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import stem_kernel_amd as ska
from stem_kernel_amd import _lib
from tests import la_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout absent")


def load_fixture():
    with open(os.path.join(ROOT, "tests", "golden", "la_protein.json")) as f:
        fx = json.load(f)
    fx["n"] = len(fx["examples"])
    for p in fx["params"]:
        for k in ("gap", "ext", "beta"):
            p[k] = float.fromhex(p[k])
        p["table"] = [float.fromhex(t) for t in p["table"]]
    fx["K"] = [[np.array([float.fromhex(v) for v in mode]).reshape(fx["n"], fx["n"]) for mode in s]
               for s in fx["values"]]
    return fx


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_la", os.path.join(ROOT, "tools", "make_golden_la.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@needs_ref
def test_fixture_is_the_references_output_bit_for_bit(tmp_path):
    gen = _generator()
    exe = gen.build_harness(REF, str(tmp_path))
    with open(os.path.join(ROOT, "tests", "golden", "la_protein.json")) as f:
        fx = json.load(f)
    ex, params = gen.examples(), gen.parameter_sets()
    assert fx["examples"] == ex
    for p, q in zip(fx["params"], params):
        assert [float.fromhex(p[k]) for k in ("gap", "ext", "beta")] == [q["gap"], q["ext"], q["beta"]]
        assert [float.fromhex(t) for t in p["table"]] == q["table"]
    assert fx["values"] == gen.reference_values(exe, str(tmp_path), ex, params)


def test_fixture_holds_the_cases(fixture):
    lens = [len(r[0]) for r in fixture["examples"] if len(r) == 1]
    assert lens[:13] == [1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200]
    odd = fixture["examples"][13][0]
    assert all(c in odd for c in "BZXU*-") and any(c.islower() for c in odd)
    two, three, same = fixture["examples"][14:17]
    assert (len(two), len(three), len(same)) == (2, 3, 3)
    assert any(all(r[k] == "-" for r in two) for k in range(len(two[0])))
    assert any(all(r[k] == "-" for r in three) for k in range(len(three[0])))
    assert same[0] == same[1] == same[2] == fixture["examples"][5][0]
    t = np.array(fixture["params"][1]["table"]).reshape(23, 23)
    assert not np.array_equal(t, t.T) and np.any(t != np.rint(t))
    assert len(fixture["values"]) == 2 and all(len(m) == fixture["n"] ** 2 for s in fixture["values"] for m in s)


@needs_ref
def test_blosum62_default_equals_the_references_table():
    rows = []
    with open(os.path.join(REF, "bpla_kernel", "la_main.cpp")) as f:
        for line in f.read().split("\n")[22:45]:  # la_main.cpp:23-45
            rows.append([float(v) for v in re.findall(r"-?\d+", line[line.index("{"):line.index("}")])])
    assert len(rows) == 23 and all(len(r) == 23 for r in rows)
    got = np.array(ska.LAKernel().params.aa_score_table[:]).reshape(23, 23)
    assert np.array_equal(got, np.array(rows))


def test_blosum62_default_is_symmetric_in_char2aa_order():
    for SW in (False, True):
        t = np.array(ska.LAKernel(SW=SW).params.aa_score_table[:]).reshape(23, 23)
        assert np.array_equal(t, t.T)
    aa = {c: k for k, c in enumerate(_lib.AA_LETTERS)}
    assert _lib.AA_LETTERS == la_ref.AA_LETTERS == "ARNDCQEGHILKMFPSTWYVBZX"
    # well-known entries of the published matrix
    for a, b, v in (("W", "W", 11), ("C", "C", 9), ("A", "A", 4), ("W", "C", -2), ("I", "V", 3), ("D", "B", 4),
                    ("E", "Z", 4), ("X", "X", -1), ("G", "I", -4), ("F", "Y", 3)):
        assert t[aa[a], aa[b]] == v
    L = _lib.lib()
    for c in range(256):
        assert L.sk_char2aa(c) == la_ref.char2aa(chr(c))
    assert L.sk_char2aa(-1) == 23 and L.sk_char2aa(1 << 20) == 23


def test_numpy_restatement_equals_the_fixture_bit_for_bit(fixture):
    cnt = [la_ref.counts(r) for r in fixture["examples"]]
    n = fixture["n"]
    for s, p in enumerate(fixture["params"]):
        for mode in range(2):
            got = np.array([[la_ref.kernel_profiles(cnt[x], cnt[y], p["table"], p["gap"], p["ext"], p["beta"],
                                                    sw=bool(mode)) for y in range(n)] for x in range(n)])
            assert np.array_equal(got, fixture["K"][s][mode]), (s, mode)


def _dataset(examples):
    ds = ska.Dataset()
    for k, rows in enumerate(examples):
        ds.add_protein(f"e{k}", rows)
    return ds


def test_aa_profile_equals_the_restatements_counts(fixture):
    ds = _dataset(fixture["examples"])
    for i, rows in enumerate(fixture["examples"]):
        prof, ns = ds.aa_profile(i)
        ref = la_ref.counts(rows)
        assert np.array_equal(prof, ref)
        assert ns == len(rows)
        assert np.all(prof.sum(axis=1) == len(rows))
    # everything that is none of the 23 letters is counted in slot 23
    prof, _ = ds.aa_profile(13)
    odd = fixture["examples"][13][0]
    assert prof[:, 23].sum() == sum(c.upper() not in la_ref.AA_LETTERS for c in odd) > 0
    # an RNA example has no amino-acid profile
    rna = ska.Dataset()
    rna.add("+1", ["ACGU"], use_bp=False)
    with pytest.raises(ska.StemKernelError):
        rna.aa_profile(0)


def test_unequal_rows_are_refused():
    ds = ska.Dataset()
    with pytest.raises(ska.StemKernelError) as e:
        ds.add_protein("+1", ["ACDE", "ACD"])
    assert e.value.code == -1 and len(ds) == 0


def test_rna_and_protein_examples_do_not_mix():
    ds = ska.Dataset()
    ds.add_protein("+1", ["ACDEFG"])
    with pytest.raises(ska.StemKernelError) as e:
        ds.add("+1", ["ACGU"], use_bp=False)
    assert e.value.code == -1
    with pytest.raises(ska.StemKernelError):
        ds.add("+1", ["ACGU"])
    rna = ska.Dataset()
    rna.add("+1", ["ACGU"], use_bp=False)
    with pytest.raises(ska.StemKernelError) as e:
        rna.add_protein("+1", ["ACDEFG"])
    assert e.value.code == -1
    # copies and imports obey the same rule
    with pytest.raises(ska.StemKernelError):
        _lib.check(_lib.lib().sk_dataset_add_copy(rna.handle, ds.handle, 0))
    with pytest.raises(ska.StemKernelError):
        rna.import_bytes(ds.export())
    with pytest.raises(ska.StemKernelError):
        ds.import_bytes(rna.export())
    assert len(ds) == 1 and len(rna) == 1


def test_4096_rows_are_refused():
    ds = ska.Dataset()
    with pytest.raises(ska.StemKernelError) as e:
        ds.add_protein("+1", ["ACD"] * 4096)
    assert e.value.code == -6
    ds.add_protein("+1", ["ACD"] * 4095)
    assert ds.aa_profile(0)[1] == 4095.0


def test_export_import_round_trip_packs_identically(fixture):
    ds = _dataset(fixture["examples"])
    blob = ds.export()
    # gathered in shares, as ranks would build them
    parts = ska.Dataset()
    parts.import_bytes(ds.export(0, 9))
    parts.import_bytes(ds.export(9))
    whole = ska.Dataset().import_bytes(blob)
    assert len(whole) == len(parts) == len(ds)
    assert [whole.label(i) for i in range(len(ds))] == [ds.label(i) for i in range(len(ds))]
    assert whole.pack_digest() == parts.pack_digest() == ds.pack_digest()
    for i in range(len(ds)):
        assert np.array_equal(whole.aa_profile(i)[0], ds.aa_profile(i)[0])
    # the digest sees the examples
    other = _dataset(fixture["examples"][:-1] + [["ACDEFGHIKL"]])
    assert other.pack_digest() != ds.pack_digest()


def test_import_rejects_one_corrupted_count():
    ds = ska.Dataset()
    ds.add_protein("+1", ["ACDWY", "ACDWW"])
    blob = ds.export()
    one, two = struct.pack("<f", 1.0), struct.pack("<f", 2.0)
    at = bytes(blob).rindex(one)  # a count of the last column
    for bad in (two, struct.pack("<f", 0.5), struct.pack("<f", -1.0)):
        broken = bytearray(blob)
        broken[at:at + 4] = bad
        fresh = ska.Dataset()
        with pytest.raises(ska.StemKernelError) as e:
            fresh.import_bytes(broken)
        assert e.value.code == -1 and len(fresh) == 0
    assert len(ska.Dataset().import_bytes(blob)) == 1


def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "stem_kernel.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in ("sk_dataset_add_protein", "sk_dataset_aa_profile", "sk_char2aa", "sk_last_la_protein"):
        assert re.search(r"\b%s\(" % name, header)
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert "SK_AA_LA = 14" in header and "SK_AA_LA_SW = 15" in header
    assert "#define SK_ABI_VERSION 3" in header
    assert re.search(r"double aa_score_table\[529\];\s*\} sk_kernel_params;", header)
    assert (_lib.AA_LA, _lib.AA_LA_SW) == (14, 15)
    assert _lib.KernelParams._fields_[-1][0] == "aa_score_table"
    assert C.sizeof(_lib.KernelParams) == _lib.KernelParams.aa_score_table.offset + 529 * 8
    for name in ("LAKernel",):
        assert hasattr(ska, name)
    assert hasattr(ska.Dataset, "add_protein") and hasattr(ska.Dataset, "aa_profile")


def test_la_kernel_defaults_are_the_cli_floats():
    p = ska.LAKernel().params
    assert p.kind == 14 and ska.LAKernel(SW=True).params.kind == 15
    assert p.gap == -10.0 and p.ext == -1.0 and p.beta == float(np.float32(0.11))
    q = ska.LAKernel(gap=-6.5, ext=-0.5, beta=0.25, score_table=np.arange(529.0)).params
    assert (q.gap, q.ext, q.beta) == (-6.5, -0.5, 0.25) and list(q.aa_score_table) == list(range(529))
    # the RNA kinds' defaults are what they were
    b = ska.BPLAKernel().params
    assert b.gap == -8.0 and b.ext == -0.75 and b.alpha == 4.5


def test_add_file_reads_protein_fasta_clustal_and_maf(tmp_path):
    fa = tmp_path / "p.fa"
    fa.write_text(">a\nMKVLAAGIWY\nHQRST\n>b\nacdefghiklmnpqrstvwyBZX*\n")
    aln = tmp_path / "p.aln"
    aln.write_text("CLUSTAL W (1.83) multiple sequence alignment\n\n"
                   "s1      MKV-LAAGIWYBZX\ns2      MKVQLA-GIWFBZX\n\n")
    maf = tmp_path / "p.maf"
    maf.write_text("##maf version=1\na score=1.0\ns p.a 0 9 + 20 MKVLA-GIWY\ns p.b 0 9 + 20 MKV-AAGIWF\n\n")
    ds = ska.Dataset()
    assert ds.add_file("+1", str(fa), "fa", protein=True) == 2
    assert ds.add_file("-1", str(aln), "aln", protein=True) == 1
    assert ds.add_file("-1", str(maf), "maf", protein=True) == 1
    assert np.array_equal(ds.aa_profile(0)[0], la_ref.counts("MKVLAAGIWYHQRST"))
    assert np.array_equal(ds.aa_profile(1)[0], la_ref.counts("acdefghiklmnpqrstvwyBZX*"))
    assert np.array_equal(ds.aa_profile(2)[0], la_ref.counts(["MKV-LAAGIWYBZX", "MKVQLA-GIWFBZX"]))
    assert np.array_equal(ds.aa_profile(3)[0], la_ref.counts(["MKVLA-GIWY", "MKV-AAGIWF"]))


def build_dropin(tmp_path, name="la_dropin"):
    libdir = os.path.join(ROOT, "stem_kernel_amd")
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-L", libdir, "-lstem_kernel_amd",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    return exe


def test_la_dropin_main_compiles(tmp_path):
    """tests/cpp/la_dropin.cpp, the body of la_main.cpp:118-135 with the one
    include swapped for include/bpla_kernel_compat.hpp."""
    assert os.path.exists(build_dropin(tmp_path))
