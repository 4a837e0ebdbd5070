"""Inputs and helpers shared by the tests that compare the oracle
(tests/test_oracle_dp_pinning.py) and the HIP kernels
(tests/test_reference_parity.py) with the reference's own DP code
(oracle/_ref/libskref_{lite,4d,str,bpla}.so, built by oracle/Makefile).

The inputs are the suite's small mixed sets: tests/test_gamma.py::_inputs
(single sequences, gapless 2- and 3-row and gapped 2-row alignments, L 64),
the short members of tests/test_string_fast.py::_items (IUPAC codes, a gapped
3-row alignment, an alignment with an all-gap column) and the tiny and ragged
BPLA set of tests/test_bpla_grad.py, plus an example whose DAG is empty."""
import functools

import numpy as np

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests.helpers import mutate_alignment

LITE_KINDS = range(8)  # SuStem SiStem SuStr SiStr SuStemStr SiStemStr LSuStem LSuStemStr


def need_reference_dp():
    """Load all four libraries.  A missing or unloadable library is an error
    whenever the reference tree or oracle/_ref is there; only with both absent
    (a checkout that never saw the reference) may the caller skip."""
    if not po.reference_dp_expected():
        return False
    for which in po.REF_DP_SOS:
        po.reference_dp(which)
    return True


def lite_items():
    base = ska.random_sequences(4, 64, 0x6A44A)
    s = ska.random_sequences(6, 150, 0x5EED0B00)
    return [base[0], mutate_alignment(base[1], 3, 0x6A44B, gap=0.0),
            mutate_alignment(base[2], 2, 0x6A44C), base[3],
            mutate_alignment(base[0], 2, 0x6A44D, gap=0.0),
            s[3][:20], "ACGUNRYKMSWACGUACGGGAAACCCRY", mutate_alignment(s[4][:40], 3, 7),
            ["ACG-UAGC", "ACG-UUGC"], ["GGGAAAUCC", "GG-AAAUCC", "GGGAAA-CC"],
            "AAAAAAAAAAAA"]  # the last: nothing pairs, the DAG is empty


def rows_of(ex):
    return [ex] if isinstance(ex, str) else list(ex)


def fold_rows(rows):
    return [ska.fold(r.replace("-", "").lower()) for r in rows]


@functools.lru_cache(maxsize=None)
def lite_examples(th, use_bp=True):
    """(oracle examples, reference examples) of lite_items(), built once."""
    om, rm = [], []
    for ex in lite_items():
        rows = rows_of(ex)
        bpps = fold_rows(rows) if use_bp else None
        om.append(po.OMData(rows, bpps, th, use_bp))
        rm.append(po.RMData(rows, bpps, th, use_bp))
    return om, rm


def lite_kernel(kind, band):
    """The product's kernel object of lite kind 0..7 with a non-default value
    of every parameter that kind reads; its .params feeds the oracle
    (po.kernel_value) and the reference (po.ref_kernel_value) alike."""
    stem = dict(loop_gap=0.35, len_band=band)
    su = dict(stem, beta=0.45)
    si = dict(stem, stack=1.15, covar=0.65)
    sus = dict(gap=0.7, alpha=0.3)
    sis = dict(gap=0.7, match=1.1, mismatch=0.6)
    return [lambda: ska.SuStemKernel(**su),
            lambda: ska.SiStemKernel(**si),
            lambda: ska.StringKernel(**sus),
            lambda: ska.StringKernel(**sis),
            lambda: ska.SuStemStrKernel(**sus, **su),
            lambda: ska.SiStemStrKernel(**sis, **si),
            lambda: ska.LSuStemKernel(**su),
            lambda: ska.LSuStemStrKernel(**sus, **su)][kind]()


def stem4d_seqs():
    return ska.random_sequences(3, 24, 99) + ["GGGAAACCC", "ACGUACGUACGUACG", "A"]


def bpla_alignments():
    alns = [mutate_alignment(s, 3, 41 + k) for k, s in enumerate(ska.random_sequences(4, 45, 41))]
    alns += [[s] for s in ska.random_sequences(2, 20, 43)]
    alns += [["ACGU-ACGUA", "ACGUAACG-A"], ["A"], ["AC", "A-"], ["GGGAAACCC"],
             ["GGGAAAUCC", "GG-AAAUCC", "GGGAAA-CC"], ["ACGUNRYKMSWACGU"]]
    return alns


def worst_rel(got, ref):
    """Largest relative difference; entries that are not finite in the
    reference (log of a zero kernel, NaN posteriors) must match exactly."""
    got = np.asarray(got, dtype=np.float64).ravel()
    ref = np.asarray(ref, dtype=np.float64).ravel()
    fin = np.isfinite(ref)
    if not np.array_equal(got[~fin], ref[~fin], equal_nan=True):
        return np.inf
    if not fin.any():
        return 0.0
    g, r = got[fin], ref[fin]
    d = np.abs(g - r)
    return float(np.max(np.where(r != 0.0, d / np.maximum(np.abs(r), 1e-300), d)))
