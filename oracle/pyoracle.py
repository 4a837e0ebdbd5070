"""ctypes loader for the CPU ORACLE (oracle/liboracle.so) and the partial
reference builds (oracle/_ref/libskref.so and libskref_{lite,4d,str,bpla}.so).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg, always as the checker, never as the product.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_SO = os.path.join(HERE, "liboracle.so")
REF_SO = os.path.join(HERE, "_ref", "libskref.so")

_o = None
_r = None

_D = C.POINTER(C.c_double)
_U = C.POINTER(C.c_uint32)
_F = C.POINTER(C.c_float)


def oracle():
    global _o
    if _o is None:
        if not os.path.exists(ORACLE_SO):
            raise RuntimeError(f"{ORACLE_SO} not built (make -C oracle)")
        L = C.CDLL(ORACLE_SO)
        L.orc_mdata_new.restype = C.c_void_p
        L.orc_mdata_new.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(_D), C.c_float, C.c_int]
        L.orc_mdata_free.argtypes = [C.c_void_p]
        for n in ("orc_mdata_n_nodes", "orc_mdata_n_edges", "orc_mdata_n_bpfreq",
                  "orc_mdata_seq_len", "orc_mdata_n_roots"):
            getattr(L, n).argtypes = [C.c_void_p]
            getattr(L, n).restype = C.c_int
        L.orc_mdata_nodes.argtypes = [C.c_void_p, _U, _U, _U, _U, _F, _U]
        L.orc_mdata_edges.argtypes = [C.c_void_p, _U, _U]
        L.orc_mdata_bpfreq.argtypes = [C.c_void_p, _U, _F]
        L.orc_mdata_roots.argtypes = [C.c_void_p, _U]
        L.orc_mdata_weight.argtypes = [C.c_void_p, _F]
        L.orc_mdata_profile.argtypes = [C.c_void_p, _F, _F]
        L.orc_mdata_bpp.argtypes = [C.c_void_p, _D]
        for n in ("orc_su_stem",):
            getattr(L, n).restype = C.c_double
            getattr(L, n).argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_uint]
        L.orc_si_stem.restype = C.c_double
        L.orc_si_stem.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_uint]
        L.orc_su_stem_ld.restype = C.c_double
        L.orc_su_stem_ld.argtypes = L.orc_su_stem.argtypes
        L.orc_si_stem_ld.restype = C.c_double
        L.orc_si_stem_ld.argtypes = L.orc_si_stem.argtypes
        L.orc_su_stem_tab.restype = C.c_double
        L.orc_su_stem_tab.argtypes = [C.c_void_p, C.c_void_p, _D, C.c_int, C.c_double, C.c_double, C.c_uint]
        L.orc_si_stem_tab.restype = C.c_double
        L.orc_si_stem_tab.argtypes = [C.c_void_p, C.c_void_p, _D, C.c_int, C.c_double, C.c_double,
                                      C.c_double, C.c_uint]
        L.orc_profile_string.restype = C.c_double
        L.orc_profile_string.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_double,
                                         C.c_double, C.c_double]
        L.orc_ribosum_tables.argtypes = [_F, _F]
        L.orc_char2rna.argtypes = [C.c_int]
        L.orc_char2rna.restype = C.c_int
        L.orc_bpla.restype = C.c_double
        L.orc_bpla.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double,
                               C.c_double, C.c_double, _D]
        L.orc_bpla_weights.argtypes = [C.c_void_p, _F, _F, _F]
        L.orc_stem4d.restype = C.c_double
        L.orc_stem4d.argtypes = [C.c_char_p, _D, C.c_char_p, _D, C.c_double, C.c_double,
                                 C.c_double, C.c_float, C.c_int, C.c_uint]
        L.orc_stem4d_ksum.restype = C.c_double
        L.orc_stem4d_ksum.argtypes = [C.c_char_p, _D, C.c_char_p, _D, C.c_double, C.c_double,
                                 C.c_double, C.c_float, C.c_int, C.c_uint]
        L.orc_stem4d_banded.restype = C.c_double
        L.orc_stem4d_banded.argtypes = [C.c_char_p, _D, C.c_char_p, _D, C.c_double, C.c_double,
                                        C.c_double, C.c_float, C.c_int, C.c_uint, C.c_uint]
        L.orc_stem4d_partial.restype = C.c_double
        L.orc_stem4d_partial.argtypes = [C.c_char_p, _D, C.c_char_p, _D, C.c_double, C.c_double,
                                         C.c_double, C.c_float, C.c_int, C.c_uint, C.c_uint,
                                         C.c_float, C.c_int]
        for n in ("orc_stem4d_gen", "orc_stem4d_partial_ld"):
            getattr(L, n).restype = C.c_double
            getattr(L, n).argtypes = [C.c_char_p, _D, C.c_char_p, _D, C.c_double, C.c_double,
                                      C.c_double, C.c_float, C.c_int, C.c_uint, C.c_uint, C.c_int]
        L.orc_stem4d_ld.restype = C.c_double
        L.orc_stem4d_ld.argtypes = [C.c_char_p, _D, C.c_char_p, _D, C.c_double, C.c_double,
                                    C.c_double, C.c_float, C.c_int, C.c_uint, C.c_int]
        L.orc_phmm_posterior.restype = C.c_int
        L.orc_phmm_posterior.argtypes = [C.c_char_p, C.c_char_p, C.c_int, _D]
        L.orc_alignment_constraints.restype = C.c_int
        L.orc_alignment_constraints.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.c_uint,
                                                C.c_int, _U, _U]
        L.orc_bpla_gradients.restype = C.c_double
        L.orc_bpla_gradients.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                         C.c_double, C.c_double, _D, _D]
        L.orc_naive_string.restype = C.c_double
        L.orc_naive_string.argtypes = [C.c_char_p, C.c_char_p, C.c_double]
        L.orc_profile_string_ld.restype = C.c_double
        L.orc_profile_string_ld.argtypes = L.orc_profile_string.argtypes
        L.orc_naive_string_ld.restype = C.c_double
        L.orc_naive_string_ld.argtypes = L.orc_naive_string.argtypes
        L.orc_profile_string_tab.restype = C.c_double
        L.orc_profile_string_tab.argtypes = [C.c_void_p, C.c_void_p] + [C.c_void_p] * 4 + \
            [C.c_int, C.c_double, C.c_double, C.c_double]
        L.orc_naive_string_tab.restype = C.c_double
        L.orc_naive_string_tab.argtypes = [C.c_char_p, C.c_char_p, C.c_double] + [C.c_void_p] * 4
        _o = L
    return _o


def reference_partial():
    """The reference's own rna.cpp/profile.cpp/ribosum.cpp (None if absent)."""
    global _r
    if _r is None:
        if not os.path.exists(REF_SO):
            return None
        L = C.CDLL(REF_SO)
        L.skref_char2rna.argtypes = [C.c_int]
        L.skref_char2rna.restype = C.c_int
        L.skref_profile.argtypes = [C.c_int, C.POINTER(C.c_char_p), _F, _F]
        L.skref_profile.restype = C.c_int
        L.skref_ribosum.argtypes = [_F, _F]
        _r = L
    return _r


# ------------------------------------------------ the reference's own DP code
# oracle/_ref/libskref_{lite,4d,str,bpla}.so: the reference's DP translation
# units compiled in place by oracle/Makefile, one library per reference tool.
REF_DP_SOS = {k: os.path.join(HERE, "_ref", f"libskref_{k}.so") for k in ("lite", "4d", "str", "bpla")}
_rdp = {}
_P = C.c_void_p


def _bind_lite(L):
    L.skl_data_new.restype = _P
    L.skl_data_new.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(_D), _D, C.c_float, C.c_int]
    L.skl_data_free.argtypes = [_P]
    for n in ("skl_n_nodes", "skl_seq_len", "skl_n_weight", "skl_n_roots", "skl_n_edges",
              "skl_n_bpfreq"):
        getattr(L, n).argtypes = [_P]
        getattr(L, n).restype = C.c_int
    L.skl_nodes.argtypes = [_P, _U, _U, _U, _U, _F, _U]
    L.skl_edges.argtypes = [_P, _U, _U]
    L.skl_bpfreq.argtypes = [_P, _U, _F]
    L.skl_roots.argtypes = [_P, _U]
    L.skl_weight.argtypes = [_P, _F]
    L.skl_kernel.restype = C.c_double
    L.skl_kernel.argtypes = [C.c_int, _P, _P, _D, C.c_uint]


def _bind_4d(L):
    L.sk4_kernel.restype = C.c_double
    L.sk4_kernel.argtypes = [C.c_char_p, _D, C.c_char_p, _D, C.c_double, C.c_double, C.c_double,
                             C.c_float, C.c_int, C.c_uint, C.c_uint, C.c_float]
    L.sk4_phmm_posterior.argtypes = [C.c_char_p, C.c_char_p, _D]
    L.sk4_alignment_constraints.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.c_uint, _U, _U]


def _bind_str(L):
    L.sks_kernel.restype = C.c_double
    L.sks_kernel.argtypes = [C.c_char_p, C.c_char_p, C.c_double]


def _bind_bpla(L):
    L.skb_data_new.restype = _P
    L.skb_data_new.argtypes = [C.c_int, C.POINTER(C.c_char_p), _D, C.c_int]
    L.skb_data_free.argtypes = [_P]
    L.skb_seq_len.argtypes = [_P]
    L.skb_seq_len.restype = C.c_int
    L.skb_weights.argtypes = [_P, _F, _F, _F]
    L.skb_kernel.restype = C.c_double
    L.skb_kernel.argtypes = [_P, _P, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                             C.c_double, _D]
    L.skb_gradients.restype = C.c_double
    L.skb_gradients.argtypes = [_P, _P, C.c_double, C.c_double, C.c_double, C.c_double, _D, _D]


def reference_dp(which: str):
    """The reference's own DP code for one tool: 'lite' (stem_kernel_lite),
    '4d' (stem_kernel with the PairHMM), 'str' (string_kernel) or 'bpla'
    (bpla_kernel).  Raises if the library is missing or does not load."""
    if which not in _rdp:
        path = REF_DP_SOS[which]
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not built (make -C oracle, with the reference present)")
        L = C.CDLL(path)
        {"lite": _bind_lite, "4d": _bind_4d, "str": _bind_str, "bpla": _bind_bpla}[which](L)
        _rdp[which] = L
    return _rdp[which]


def reference_dp_expected() -> bool:
    """True when the reference DP libraries must exist: the reference tree or
    a built oracle/_ref is present (only with both absent may a test skip)."""
    return os.path.isdir("/root/reference") or os.path.isdir(os.path.join(HERE, "_ref"))


def _packed_ptr(b):
    b = np.ascontiguousarray(b, dtype=np.float64)
    if b.size == 0:
        b = np.zeros(1)
    return b


class RMData:
    """One example built by the reference's own Data constructor
    (stem_kernel_lite/data.cpp) from injected base-pairing probabilities:
    the per-row packed matrices the oracle takes, and the oracle's averaged
    table (the averaging itself is not part of the reference build)."""

    def __init__(self, rows: Sequence[str], bpp_rows, th=0.01, use_bp=True, avg=None):
        L = reference_dp("lite")
        n = len(rows)
        self._rows = (C.c_char_p * n)(*[r.encode() for r in rows])
        self._keep = []
        barr = (_D * n)()
        a = None
        if use_bp:
            for k, b in enumerate(bpp_rows):
                b = _packed_ptr(b)
                self._keep.append(b)
                barr[k] = b.ctypes.data_as(_D)
            if avg is None:
                om = OMData(rows, bpp_rows, th)
                sl = oracle().orc_mdata_seq_len(om.h)
                avg = np.zeros(max(sl * (sl - 1) // 2, 1))
                oracle().orc_mdata_bpp(om.h, avg.ctypes.data_as(_D))
            a = _packed_ptr(avg)
            self._keep.append(a)
        self.h = _P(L.skl_data_new(n, self._rows, barr, a.ctypes.data_as(_D) if a is not None else None,
                                   C.c_float(th), int(use_bp)))

    def __del__(self):
        if getattr(self, "h", None) and "lite" in _rdp:
            _rdp["lite"].skl_data_free(self.h)
            self.h = None

    def dag(self) -> dict:
        L = reference_dp("lite")
        nn, ne, nb = L.skl_n_nodes(self.h), L.skl_n_edges(self.h), L.skl_n_bpfreq(self.h)
        nr, nw = L.skl_n_roots(self.h), L.skl_n_weight(self.h)
        u = lambda k: np.zeros(max(k, 1), np.uint32)
        f = lambda k: np.zeros(max(k, 1), np.float32)
        first, last, ned, nbf, mp = u(nn), u(nn), u(nn), u(nn), u(nn)
        w = f(nn)
        L.skl_nodes(self.h, *(a.ctypes.data_as(_U) for a in (first, last, ned, nbf)),
                    w.ctypes.data_as(_F), mp.ctypes.data_as(_U))
        to, gaps = u(ne), u(ne)
        L.skl_edges(self.h, to.ctypes.data_as(_U), gaps.ctypes.data_as(_U))
        code, p = u(nb), f(nb)
        L.skl_bpfreq(self.h, code.ctypes.data_as(_U), p.ctypes.data_as(_F))
        roots = u(nr)
        L.skl_roots(self.h, roots.ctypes.data_as(_U))
        pw = f(nw)
        L.skl_weight(self.h, pw.ctypes.data_as(_F))
        return dict(first=first[:nn], last=last[:nn], n_edges=ned[:nn], n_bpfreq=nbf[:nn],
                    weight=w[:nn], max_pa=mp[:nn], edge_to=to[:ne], edge_gaps=gaps[:ne],
                    bp_code=code[:nb], bp_p=p[:nb], roots=roots[:nr], pos_weight=pw[:nw])


def ref_kernel_value(kind: int, x: RMData, y: RMData, p) -> float:
    """K(x, y) of lite kind 0..7 by the reference's own kernel classes
    (def_kernel.h); p is a KernelParams-like object."""
    v = (C.c_double * 8)(p.loop_gap, p.beta, p.stack, p.covar, p.gap, p.alpha, p.match, p.mismatch)
    return reference_dp("lite").skl_kernel(kind, x.h, y.h, v, int(p.len_band))


def ref_naive_string(x: str, y: str, gap=0.8) -> float:
    return reference_dp("str").sks_kernel(x.encode(), y.encode(), gap)


def ref_stem4d(x: str, bpx, y: str, bpy, gap=0.8, stack=1.0, subst=0.5, bp_bound=0.0, model=0,
               loop=3, band=0, ali_bound=0.0) -> float:
    """The reference's StemKernel::operator() (stem_kernel/stem_kernel.h)."""
    keep = [np.ascontiguousarray(b, dtype=np.float64) if b is not None else None for b in (bpx, bpy)]
    px = keep[0].ctypes.data_as(_D) if keep[0] is not None and keep[0].size else None
    py = keep[1].ctypes.data_as(_D) if keep[1] is not None and keep[1].size else None
    return reference_dp("4d").sk4_kernel(x.encode(), px, y.encode(), py, gap, stack, subst,
                                         bp_bound, model, loop, band, ali_bound)


def ref_phmm_posterior(x: str, y: str) -> np.ndarray:
    fb = np.zeros((3, len(x) + 1, len(y) + 1))
    reference_dp("4d").sk4_phmm_posterior(x.encode(), y.encode(), fb.ctypes.data_as(_D))
    return fb


def ref_alignment_constraints(x: str, y: str, ali_bound: float, band=0):
    lo = np.zeros(len(x) + 1, np.uint32)
    hi = np.zeros(len(x) + 1, np.uint32)
    reference_dp("4d").sk4_alignment_constraints(x.encode(), y.encode(), ali_bound, band,
                                                 lo.ctypes.data_as(_U), hi.ctypes.data_as(_U))
    return lo, hi


class RBData:
    """One BPLA example built by the reference's own Data constructor
    (bpla_kernel/data.cpp: fill_weight) on the injected averaged table."""

    def __init__(self, rows: Sequence[str], bpp_rows, use_bp=True):
        L = reference_dp("bpla")
        n = len(rows)
        self._rows = (C.c_char_p * n)(*[r.encode() for r in rows])
        a = None
        if use_bp:
            om = OMData(rows, bpp_rows, 0.01)
            sl = oracle().orc_mdata_seq_len(om.h)
            a = np.zeros(max(sl * (sl - 1) // 2, 1))
            oracle().orc_mdata_bpp(om.h, a.ctypes.data_as(_D))
        self._keep = a
        self.h = _P(L.skb_data_new(n, self._rows, a.ctypes.data_as(_D) if a is not None else None,
                                   int(use_bp)))

    def __del__(self):
        if getattr(self, "h", None) and "bpla" in _rdp:
            _rdp["bpla"].skb_data_free(self.h)
            self.h = None

    def weights(self):
        L = reference_dp("bpla")
        n = L.skb_seq_len(self.h)
        a = [np.zeros(max(n, 1), np.float32) for _ in range(3)]
        L.skb_weights(self.h, *(v.ctypes.data_as(_F) for v in a))
        return [v[:n] for v in a]


def ref_bpla(x: RBData, y: RBData, no_bp: bool, sw: bool, gap, ext, alpha, beta, table16) -> float:
    t = (C.c_double * 16)(*table16)
    return reference_dp("bpla").skb_kernel(x.h, y.h, int(no_bp), int(sw), gap, ext, alpha, beta, t)


def ref_bpla_gradients(x: RBData, y: RBData, alpha, beta, gap, ext, table16):
    t = np.ascontiguousarray(table16, dtype=np.float64)
    d = np.zeros(4)
    v = reference_dp("bpla").skb_gradients(x.h, y.h, alpha, beta, gap, ext, t.ctypes.data_as(_D),
                                           d.ctypes.data_as(_D))
    return v, d


class OMData:
    """Oracle MData (one example)."""

    def __init__(self, rows: Sequence[str], bpp_rows: Optional[Sequence[np.ndarray]], th=0.01,
                 use_bp=True):
        L = oracle()
        n = len(rows)
        self._rows = (C.c_char_p * n)(*[r.encode() for r in rows])
        self._keep = []
        barr = (_D * n)()
        if use_bp:
            for k, b in enumerate(bpp_rows):
                b = np.ascontiguousarray(b, dtype=np.float64)
                if b.size == 0:
                    b = np.zeros(1)
                self._keep.append(b)
                barr[k] = b.ctypes.data_as(_D)
        self.h = C.c_void_p(L.orc_mdata_new(n, self._rows, barr, C.c_float(th), int(use_bp)))

    def __del__(self):
        if getattr(self, "h", None) and _o is not None:
            _o.orc_mdata_free(self.h)
            self.h = None

    def dag(self) -> dict:
        L = oracle()
        nn = L.orc_mdata_n_nodes(self.h)
        ne = L.orc_mdata_n_edges(self.h)
        nb = L.orc_mdata_n_bpfreq(self.h)
        nr = L.orc_mdata_n_roots(self.h)
        sl = L.orc_mdata_seq_len(self.h)
        u = lambda k: np.zeros(max(k, 1), np.uint32)
        f = lambda k: np.zeros(max(k, 1), np.float32)
        first, last, ned, nbf, mp = u(nn), u(nn), u(nn), u(nn), u(nn)
        w = f(nn)
        L.orc_mdata_nodes(self.h, *(a.ctypes.data_as(_U) for a in (first, last, ned, nbf)),
                          w.ctypes.data_as(_F), mp.ctypes.data_as(_U))
        to, gaps = u(ne), u(ne)
        L.orc_mdata_edges(self.h, to.ctypes.data_as(_U), gaps.ctypes.data_as(_U))
        code, p = u(nb), f(nb)
        L.orc_mdata_bpfreq(self.h, code.ctypes.data_as(_U), p.ctypes.data_as(_F))
        roots = u(nr)
        L.orc_mdata_roots(self.h, roots.ctypes.data_as(_U))
        pw = f(sl)
        L.orc_mdata_weight(self.h, pw.ctypes.data_as(_F))
        return dict(first=first[:nn], last=last[:nn], n_edges=ned[:nn], n_bpfreq=nbf[:nn],
                    weight=w[:nn], max_pa=mp[:nn], edge_to=to[:ne], edge_gaps=gaps[:ne],
                    bp_code=code[:nb], bp_p=p[:nb], roots=roots[:nr], pos_weight=pw[:sl])


def su_stem(x: OMData, y: OMData, loop_gap=0.2, beta=0.3, band=10) -> float:
    return oracle().orc_su_stem(x.h, y.h, loop_gap, beta, band)


def si_stem(x: OMData, y: OMData, loop_gap=0.2, stack=1.3, covar=0.8, band=10) -> float:
    return oracle().orc_si_stem(x.h, y.h, loop_gap, stack, covar, band)


def su_stem_ld(x: OMData, y: OMData, loop_gap=0.2, beta=0.3, band=10) -> float:
    """su_stem with the DP's products and sums in long double (same tables),
    rounded to double once."""
    return oracle().orc_su_stem_ld(x.h, y.h, loop_gap, beta, band)


def si_stem_ld(x: OMData, y: OMData, loop_gap=0.2, stack=1.3, covar=0.8, band=10) -> float:
    return oracle().orc_si_stem_ld(x.h, y.h, loop_gap, stack, covar, band)


def gap_weights(loop_gap: float, n: int) -> np.ndarray:
    """The oracle's gap-power table: w[0] = 1, w[k] = w[k-1] * loop_gap."""
    w = np.empty(max(n, 1))
    w[0] = 1.0
    for k in range(1, w.size):
        w[k] = w[k - 1] * loop_gap
    return w


def su_stem_tab(x: OMData, y: OMData, w, gap2: float, beta=0.3, band=10) -> float:
    """su_stem (double) with the gap-weight table w[k] in place of loop_gap^k
    and gap2 in place of loop_gap^2 in the node gap score."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    return oracle().orc_su_stem_tab(x.h, y.h, w.ctypes.data_as(_D), w.size, gap2, beta, band)


def si_stem_tab(x: OMData, y: OMData, w, gap2: float, stack=1.3, covar=0.8, band=10) -> float:
    w = np.ascontiguousarray(w, dtype=np.float64)
    return oracle().orc_si_stem_tab(x.h, y.h, w.ctypes.data_as(_D), w.size, gap2, stack, covar, band)


def su_str(x: OMData, y: OMData, gap=0.8, alpha=0.2) -> float:
    return oracle().orc_profile_string(x.h, y.h, gap, 1, alpha, 0.0, 0.0)


def si_str(x: OMData, y: OMData, gap=0.8, match=1.0, mismatch=0.8) -> float:
    return oracle().orc_profile_string(x.h, y.h, gap, 0, 0.0, match, mismatch)


def _log(v: float) -> float:
    """C's log, as LogKernel (conv_kernel.h) calls it: -inf at 0 (a pair with
    an empty DAG), where math.log raises."""
    import math
    return math.log(v) if v > 0.0 else (-math.inf if v == 0.0 else math.nan)


def kernel_value(kind: int, x: OMData, y: OMData, p) -> float:
    """Composite kernels of def_kernel.h / conv_kernel.h from the components;
    p is a KernelParams-like object (attribute access)."""
    stem = lambda: su_stem(x, y, p.loop_gap, p.beta, p.len_band)
    if kind == 0:
        return stem()
    if kind == 1:
        return si_stem(x, y, p.loop_gap, p.stack, p.covar, p.len_band)
    if kind == 2:
        return su_str(x, y, p.gap, p.alpha)
    if kind == 3:
        return si_str(x, y, p.gap, p.match, p.mismatch)
    if kind == 4:
        return stem() + su_str(x, y, p.gap, p.alpha)
    if kind == 5:
        return si_stem(x, y, p.loop_gap, p.stack, p.covar, p.len_band) + si_str(x, y, p.gap, p.match, p.mismatch)
    if kind == 6:
        return p.beta * _log(stem()) + 0.0
    if 9 <= kind <= 12:
        return bpla(x, y, kind in (10, 12), kind in (11, 12), p.gap, p.ext, p.alpha, p.beta,
                    list(p.score_table))
    if kind == 8:
        raise ValueError("naive string kernel compares raw strings: use naive_string()")
    if kind == 7:
        return (p.beta * _log(stem()) + 0.0) + (p.alpha * _log(su_str(x, y, p.gap, p.alpha)) + 0.0)
    raise ValueError(kind)


def naive_string(x: str, y: str, gap=0.8) -> float:
    return oracle().orc_naive_string(x.encode(), y.encode(), gap)


def su_str_ld(x: OMData, y: OMData, gap=0.8, alpha=0.2) -> float:
    """su_str with the DP's products and sums in long double (the same per-cell
    factors and gap), rounded to double once."""
    return oracle().orc_profile_string_ld(x.h, y.h, gap, 1, alpha, 0.0, 0.0)


def si_str_ld(x: OMData, y: OMData, gap=0.8, match=1.0, mismatch=0.8) -> float:
    return oracle().orc_profile_string_ld(x.h, y.h, gap, 0, 0.0, match, mismatch)


def naive_string_ld(x: str, y: str, gap=0.8) -> float:
    return oracle().orc_naive_string_ld(x.encode(), y.encode(), gap)


def string_tables(gap: float, lx: int, ly: int) -> dict:
    """The geometric tables of the string DPs' table twins, as long doubles by
    repeated products: R[j] = G0[0][j], C[i] = G0[i][0], wh[d] / wv[d] the
    weight of a horizontal / vertical run of d (all gap^k)."""
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError("numpy's longdouble is not the C long double of the oracle")

    def geo(n):
        w = np.empty(n + 1, dtype=np.longdouble)
        w[0] = 1
        for k in range(1, n + 1):
            w[k] = w[k - 1] * np.longdouble(gap)
        return w
    return dict(R=geo(ly), C=geo(lx), wh=geo(ly), wv=geo(lx))


def _ldp(t, n):
    t = np.ascontiguousarray(t, dtype=np.longdouble)
    if t.size < n + 1:
        raise ValueError(f"table of {t.size} entries, {n + 1} needed")
    return t


def _tabs(tab, lx, ly):
    keep = [_ldp(tab["R"], ly), _ldp(tab["C"], lx), _ldp(tab["wh"], ly), _ldp(tab["wv"], lx)]
    return keep, [C.c_void_p(t.ctypes.data) for t in keep]


def su_str_tab(x: OMData, y: OMData, tab: dict, alpha=0.2) -> float:
    """su_str over the caller's tables (string_tables) instead of gap^k."""
    keep, p = _tabs(tab, oracle().orc_mdata_seq_len(x.h), oracle().orc_mdata_seq_len(y.h))
    return oracle().orc_profile_string_tab(x.h, y.h, *p, 1, alpha, 0.0, 0.0)


def si_str_tab(x: OMData, y: OMData, tab: dict, match=1.0, mismatch=0.8) -> float:
    keep, p = _tabs(tab, oracle().orc_mdata_seq_len(x.h), oracle().orc_mdata_seq_len(y.h))
    return oracle().orc_profile_string_tab(x.h, y.h, *p, 0, 0.0, match, mismatch)


def naive_string_tab(x: str, y: str, gap: float, tab: dict) -> float:
    """naive_string over the caller's tables; gap only for the match weight gap^2."""
    keep, p = _tabs(tab, len(x), len(y))
    return oracle().orc_naive_string_tab(x.encode(), y.encode(), gap, *p)


def bpla(x: OMData, y: OMData, no_bp: bool, sw: bool, gap, ext, alpha, beta, table16) -> float:
    t = (C.c_double * 16)(*table16)
    return oracle().orc_bpla(x.h, y.h, int(no_bp), int(sw), gap, ext, alpha, beta, t)


def bpla_weights(x: OMData):
    L = oracle().orc_mdata_seq_len(x.h)
    a = [np.zeros(max(L, 1), np.float32) for _ in range(3)]
    oracle().orc_bpla_weights(x.h, *(v.ctypes.data_as(_F) for v in a))
    return [v[:L] for v in a]


def stem4d(x: str, bpx, y: str, bpy, gap=0.8, stack=1.0, subst=0.5, bp_bound=0.0, model=0,
           loop=3, band=0, ali_bound=0.0, zerop_fixed=0) -> float:
    """StemKernel::operator() of stem_kernel/stem_kernel.h:52-55: full_dp
    (stem_kernel.cpp:282-351), or partial_dp (:113-280) when band or
    ali_bound is set (x, y as the loader gives them: lowercase)."""
    def arr(b):
        if b is None:
            return None
        b = np.ascontiguousarray(b, dtype=np.float64)
        return b.ctypes.data_as(_D) if b.size else np.zeros(1).ctypes.data_as(_D)
    keep = [np.ascontiguousarray(b, dtype=np.float64) if b is not None else None for b in (bpx, bpy)]
    px = keep[0].ctypes.data_as(_D) if keep[0] is not None and keep[0].size else None
    py = keep[1].ctypes.data_as(_D) if keep[1] is not None and keep[1].size else None
    if ali_bound > 0.0:
        return oracle().orc_stem4d_partial(x.encode(), px, y.encode(), py, gap, stack, subst,
                                           bp_bound, model, loop, band, ali_bound, zerop_fixed)
    if band:
        return oracle().orc_stem4d_banded(x.encode(), px, y.encode(), py, gap, stack, subst,
                                          bp_bound, model, loop, band)
    return oracle().orc_stem4d(x.encode(), px, y.encode(), py, gap, stack, subst, bp_bound,
                               model, loop)


def _bpp_args(bpx, bpy):
    keep = [np.ascontiguousarray(b, dtype=np.float64) if b is not None else None for b in (bpx, bpy)]
    return keep, [k.ctypes.data_as(_D) if k is not None and k.size else None for k in keep]


def stem4d_ld(x: str, bpx, y: str, bpy, gap=0.8, stack=1.0, subst=0.5, bp_bound=0.0, model=0,
              loop=3, band=0, cut=-1) -> float:
    """stem4d() without -a (full_dp, or partial_dp under the -b band) with
    every product and sum in long double, rounded to double once
    (oracle/stem4d_generic.inc).  cut >= 0: the two base terms G0 = g^(l-k) and
    g^(j-i) are zero beyond cut positions (the visibility tests' emulation of
    a truncated gap-power table); cut < 0 is the DP itself."""
    keep, (px, py) = _bpp_args(bpx, bpy)
    if band:
        return oracle().orc_stem4d_partial_ld(x.encode(), px, y.encode(), py, gap, stack, subst,
                                              bp_bound, model, loop, band, cut)
    return oracle().orc_stem4d_ld(x.encode(), px, y.encode(), py, gap, stack, subst, bp_bound,
                                  model, loop, cut)


def stem4d_gen(x: str, bpx, y: str, bpy, gap=0.8, stack=1.0, subst=0.5, bp_bound=0.0, model=0,
               loop=3, band=0, cut=-1) -> float:
    """The double instantiation of stem4d_ld()'s generic body: stem4d() bit
    for bit when cut < 0 (tests/test_stem4d_oracle_twin.py)."""
    keep, (px, py) = _bpp_args(bpx, bpy)
    return oracle().orc_stem4d_gen(x.encode(), px, y.encode(), py, gap, stack, subst, bp_bound,
                                   model, loop, band, cut)


def stem4d_ksum(x: str, bpx, y: str, bpy, gap=0.8, stack=1.0, subst=0.5, bp_bound=0.0, model=0,
                loop=3) -> float:
    """full_dp's K as 1 + the sum of the stacking sources (the engine's K-sum
    formulation), from the same loops as stem4d()."""
    keep = [np.ascontiguousarray(b, dtype=np.float64) if b is not None else None for b in (bpx, bpy)]
    px = keep[0].ctypes.data_as(_D) if keep[0] is not None and keep[0].size else None
    py = keep[1].ctypes.data_as(_D) if keep[1] is not None and keep[1].size else None
    return oracle().orc_stem4d_ksum(x.encode(), px, y.encode(), py, gap, stack, subst, bp_bound,
                                    model, loop)


def phmm_posterior(x: str, y: str, zerop_fixed=0) -> np.ndarray:
    """PairHMM posteriors fb[s, i, j] (stem_kernel/phmm.cpp:10-115)."""
    fb = np.zeros((3, len(x) + 1, len(y) + 1))
    if oracle().orc_phmm_posterior(x.encode(), y.encode(), zerop_fixed, fb.ctypes.data_as(_D)):
        raise ValueError("unknown nucleotide")
    return fb


def alignment_constraints(x: str, y: str, ali_bound: float, band=0, zerop_fixed=0):
    """StemKernel::alignment_constraints (stem_kernel/stem_kernel.cpp:14-81)."""
    lo = np.zeros(len(x) + 1, np.uint32)
    hi = np.zeros(len(x) + 1, np.uint32)
    if oracle().orc_alignment_constraints(x.encode(), y.encode(), ali_bound, band, zerop_fixed,
                                          lo.ctypes.data_as(_U), hi.ctypes.data_as(_U)):
        raise ValueError("unknown nucleotide")
    return lo, hi


def bpla_gradients(x: OMData, y: OMData, alpha, beta, gap, ext, table16):
    """BPLAKernel::compute_gradients (bpla_kernel.cpp:385-401): (value,
    [d_alpha, d_beta, d_gap, d_ext], backward total)."""
    t = np.ascontiguousarray(table16, dtype=np.float64)
    d = np.zeros(5)
    v = oracle().orc_bpla_gradients(x.h, y.h, alpha, beta, gap, ext, t.ctypes.data_as(_D),
                                    d.ctypes.data_as(_D))
    return v, d[:4].copy(), float(d[4])


# ------------------------------------------------------------------ McCaskill fold
def _fold_lib():
    L = oracle()
    if not getattr(L, "_fold_bound", False):
        L.orc_fold_mccaskill.restype = C.c_double
        L.orc_fold_mccaskill.argtypes = [C.c_char_p, C.c_int, C.c_int, _D]
        L.orc_fold_enum.restype = C.c_double
        L.orc_fold_enum.argtypes = [C.c_char_p, C.c_int, C.c_int, _D, C.POINTER(C.c_long)]
        L.orc_fold_structure_energy.restype = C.c_double
        L.orc_fold_structure_energy.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_int, C.c_int]
        L._fold_bound = True
    return L


def _fl(no_closing_gu, no_lp):
    """fold_oracle.c's third argument: bit 0 --noClosingGU, bit 1 --noLonelyPairs."""
    return int(bool(no_closing_gu)) | (2 if no_lp else 0)


def fold_mccaskill(seq: str, no_gu=False, no_closing_gu=False, no_lp=False):
    """(ln Z, packed bpp) of the restated McCaskill DP (fold_oracle.c)."""
    n = len(seq)
    bpp = np.zeros(max(n * (n - 1) // 2, 1))
    lz = _fold_lib().orc_fold_mccaskill(seq.encode(), int(no_gu), _fl(no_closing_gu, no_lp),
                                        bpp.ctypes.data_as(_D))
    return lz, bpp[: n * (n - 1) // 2]


def fold_enum(seq: str, no_gu=False, no_closing_gu=False, no_lp=False):
    """(ln Z, packed bpp, number of structures) by exhaustive enumeration."""
    n = len(seq)
    bpp = np.zeros(max(n * (n - 1) // 2, 1))
    cnt = C.c_long()
    lz = _fold_lib().orc_fold_enum(seq.encode(), int(no_gu), _fl(no_closing_gu, no_lp),
                                   bpp.ctypes.data_as(_D), C.byref(cnt))
    return lz, bpp[: n * (n - 1) // 2], cnt.value


def fold_structure_energy(seq: str, dotbracket: str, no_gu=False, no_closing_gu=False) -> float:
    st, pt = [], np.full(len(seq), -1, np.int32)
    for k, c in enumerate(dotbracket):
        if c == "(":
            st.append(k)
        elif c == ")":
            i = st.pop()
            pt[i], pt[k] = k, i
    return _fold_lib().orc_fold_structure_energy(seq.encode(), pt.ctypes.data_as(C.POINTER(C.c_int)),
                                                 int(no_gu), int(no_closing_gu))
