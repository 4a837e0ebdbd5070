"""Test-only restatement of the stem DP with forward-mode tangents, in
numpy.longdouble: stem_dp of oracle/stem_dp_generic.inc
(stem_kernel_lite/stem_kernel.cpp:14-95) over OMData.dag() and the profile
accessor, every DP quantity (K0, G0, K1, G1, v_s, e_s) an array
[value, tangent per parameter], the product rule in the DP's own operation
order.  The tables are the oracle's: co_subst from the double exp, the float
bp frequencies and node weights, the double gap powers w[k] = w[k-1] * g and
gap2 = g * g; their tangents are k * w[k-1], g + g, P[c] * co_subst[c] (Su)
and the code-equality indicators (Si).  Only the DP's products and sums are
long double.

su(x, y, ...) -> [K, dK/dloop_gap, dK/dbeta]
si(x, y, ...) -> [K, dK/dloop_gap, dK/dstack, dK/dcovar]
row4(kind, r) puts the tangents into the four-slot row (loop_gap, beta,
stack, covar) of sk_stem_gradients."""
import ctypes as C
import math

import numpy as np

import stem_kernel_amd as ska
from oracle import pyoracle as po

LD = np.longdouble
_F = C.POINTER(C.c_float)


def _ribosum_p():
    s, p = np.zeros(16, np.float32), np.zeros(256, np.float32)
    ska.lib().sk_ribosum_tables(s.ctypes.data_as(_F), p.ctypes.data_as(_F))
    return p.astype(np.float64)


class Ex:
    """One oracle example's DAG and profile as plain arrays."""

    def __init__(self, om):
        d = om.dag()
        self.first, self.last = d["first"].astype(np.int64), d["last"].astype(np.int64)
        self.weight = d["weight"].astype(np.float64)
        self.n = len(self.first)
        ne, nb = d["n_edges"].astype(np.int64), d["n_bpfreq"].astype(np.int64)
        self.eoff = np.concatenate([[0], np.cumsum(ne)])
        self.boff = np.concatenate([[0], np.cumsum(nb)])
        self.to, self.gaps = d["edge_to"].astype(np.int64), d["edge_gaps"].astype(np.int64)
        self.code, self.p = d["bp_code"].astype(np.int64), d["bp_p"].astype(np.float64)
        self.roots = d["roots"].astype(np.int64)
        L = po.oracle()
        sl = L.orc_mdata_seq_len(om.h)
        prof = np.zeros(max(5 * sl, 1), np.float32)
        ns = C.c_float(0)
        L.orc_mdata_profile(om.h, prof.ctypes.data_as(_F), C.byref(ns))
        self.len = sl
        self.n_seqs = float(ns.value)
        # the profile's gap count at every node's first position
        self.nbp = np.array([float(prof[5 * f + 4]) for f in self.first]) if self.n else np.zeros(0)


def _dp(x, y, loop_gap, band, subst, beta=0.0, stack=0.0, covar=0.0):
    """The DP row by row over x; within a row every y node at once (numpy over
    the y nodes and edges, the sums of one cell in the DP's order), the y
    recurrence level by level."""
    NP = 2 if subst else 3
    T = 1 + NP
    nw = 2 * max(x.len, y.len) + 2
    w = np.ones(nw, np.float64)
    for k in range(1, nw):
        w[k] = w[k - 1] * loop_gap
    dw = np.zeros(nw, np.float64)
    for k in range(1, nw):
        dw[k] = k * w[k - 1]
    w, dw = w.astype(LD), dw.astype(LD)
    gap2, dgap2 = LD(loop_gap * loop_gap), LD(loop_gap + loop_gap)
    if subst:
        P = _ribosum_p()
        co = np.array([math.exp(P[c] * beta) for c in range(256)])
        dco = (P * co).astype(LD)
        co = co.astype(LD)
    if x.n == 0 or y.n == 0:
        return np.zeros(T, LD)
    ny = y.n
    yne = np.diff(y.eoff)
    yleaf = yne == 0
    ypar = np.repeat(np.arange(ny), yne)           # parent of every y edge
    ybpar = np.repeat(np.arange(ny), np.diff(y.boff))  # node of every y bp entry
    ylen = y.last - y.first
    yp = y.p.astype(LD)
    # y levels: children first
    lev = np.zeros(ny, np.int64)
    for j in range(ny):
        if yne[j]:
            lev[j] = 1 + max(lev[y.to[e]] for e in range(y.eoff[j], y.eoff[j + 1]))
    lev_edges = [np.flatnonzero(lev[ypar] == L) for L in range(1, int(lev.max()) + 1)] if ny else []
    # node_gap of y and its tangent
    vsy = np.zeros((ny, 2), LD)
    vsy[:, 0] = gap2 * y.weight.astype(LD)
    vsy[:, 1] = dgap2 * y.weight.astype(LD)
    ew, edw = w[y.gaps], dw[y.gaps]

    def times_gap(g, vs0, dvs, es, des):
        """g * v_s * e_s over rows: v_s, e_s depend on loop_gap alone."""
        r = g * (vs0 * es)[:, None]
        r[:, 0] = g[:, 0] * vs0 * es
        r[:, 1] = (g[:, 1] * vs0 + g[:, 0] * dvs) * es + g[:, 0] * vs0 * des
        return r

    K0 = np.zeros((x.n, ny, T), LD)
    G0 = np.zeros((x.n, ny, T), LD)
    K1 = np.zeros((ny, T), LD)
    G1 = np.zeros((ny, T), LD)
    for i in range(x.n):
        xe = range(x.eoff[i], x.eoff[i + 1])
        xleaf = len(xe) == 0
        if xleaf:
            # leaf x leaf cells are 1 (K1, G1 keep their values there); the rest
            # of the row has no match term
            M = np.zeros((ny, T), LD)
        else:
            # node_match(i, j) for every j
            vs = np.zeros((ny, T), LD)
            for a in range(x.boff[i], x.boff[i + 1]):
                cx = LD(x.p[a])
                if subst:
                    c = x.code[a] * 16 + y.code
                    np.add.at(vs[:, 0], ybpar, co[c] * cx * yp)
                    np.add.at(vs[:, 2], ybpar, dco[c] * cx * yp)
                else:
                    eq = x.code[a] == y.code
                    np.add.at(vs[:, 0], ybpar, np.where(eq, LD(stack), LD(covar)) * cx * yp)
                    np.add.at(vs[:, 2], ybpar, np.where(eq, cx * yp, LD(0)))
                    np.add.at(vs[:, 3], ybpar, np.where(eq, LD(0), cx * yp))
            vs[:, :2] += vsy * LD(x.nbp[i]) / LD(x.n_seqs)
            xg = np.array([gap2 * LD(x.weight[i]), dgap2 * LD(x.weight[i])])
            vs[:, :2] += xg[None, :] * y.nbp.astype(LD)[:, None] / LD(y.n_seqs)
            inband = np.ones(ny, bool) if band == 0 else np.abs(int(x.last[i] - x.first[i]) - ylen) <= band
            M = np.zeros((ny, T), LD)
            sel = np.flatnonzero(inband[ypar])
            par = ypar[sel]
            for ex in xe:
                gx = x.gaps[ex]
                g = G0[x.to[ex]][y.to[sel]]
                es = w[gx] * ew[sel]
                des = dw[gx] * ew[sel] + w[gx] * edw[sel]
                v = (g * vs[par, 0:1] + g[:, 0:1] * vs[par]) * es[:, None]
                v[:, 0] = g[:, 0] * vs[par, 0] * es
                v[:, 1] += g[:, 0] * vs[par, 0] * des
                np.add.at(M, par, v)
        # the y recurrence: K1[j] = M + sum K1[child], G1[j] = M + sum G1[child] v_s e_s
        nl = ~yleaf if xleaf else np.ones(ny, bool)  # cells that are not leaf x leaf
        K1[nl] = M[nl]
        G1[nl] = M[nl]
        for es_ in lev_edges:
            par, to = ypar[es_], y.to[es_]
            np.add.at(K1, par, K1[to])
            np.add.at(G1, par, times_gap(G1[to], vsy[par, 0], vsy[par, 1], ew[es_], edw[es_]))
        K0[i] = K1
        G0[i] = G1
        if xleaf:
            K0[i, yleaf] = 0
            G0[i, yleaf] = 0
            K0[i, yleaf, 0] = 1.0
            G0[i, yleaf, 0] = 1.0
        for ex in xe:
            gx = x.gaps[ex]
            K0[i] += K0[x.to[ex]]
            n1 = np.full(ny, gap2 * LD(x.weight[i]))
            n2 = np.full(ny, dgap2 * LD(x.weight[i]))
            G0[i] += times_gap(G0[x.to[ex]], n1, n2, np.full(ny, w[gx]), np.full(ny, dw[gx]))
    ret = np.zeros(T, LD)
    for a in x.roots:
        for b in y.roots:
            ret += K0[a, b]
    return ret


def su(x, y, loop_gap=0.2, beta=0.3, band=10):
    return _dp(x, y, loop_gap, band, True, beta=beta)


def si(x, y, loop_gap=0.2, stack=1.3, covar=0.8, band=10):
    return _dp(x, y, loop_gap, band, False, stack=stack, covar=covar)


def row4(subst, r):
    """The tangents of su / si in sk_stem_gradients' four-slot row."""
    g = np.zeros(4, LD)
    g[0] = r[1]
    if subst:
        g[1] = r[2]
    else:
        g[2], g[3] = r[2], r[3]
    return g


def ulp_diff(a, b):
    """|a - b| in units of the last place of b (doubles)."""
    a, b = float(a), float(b)
    if a == b:
        return 0.0
    return abs(a - b) / math.ulp(b)
