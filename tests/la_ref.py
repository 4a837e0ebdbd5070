"""numpy restatement of the reference's la_kernel, bit for bit:
BPLAKernel<double,AAMData>::operator() (bpla_kernel/bpla_kernel.cpp:159-174,
noBP) = local_alignment_exp (:64-115) or local_alignment_max (:117-157) with
LAScore (:16-45) over AAProfileSequence columns (common/aaprofile.cpp:49-60).

Every arithmetic operation is the reference's, in its order and its number
format (float32 counts and weight n, double everywhere else, no fused
multiply-add); only independent cells are evaluated together, one
anti-diagonal at a time.  exp goes through libm (math.exp), as the reference's
does.  tests/test_la_protein_cpu.py pins it to the reference through
tests/golden/la_protein.json; the GPU tests use it for random inputs."""
import math

import numpy as np

AA_LETTERS = "ARNDCQEGHILKMFPSTWYVBZX"
N_AA = 23


def char2aa(c):
    """common/aaprofile.cpp:13-23 (the C locale's toupper: ASCII only)."""
    if "a" <= c <= "z":
        c = c.upper()
    k = AA_LETTERS.find(c) if len(c) == 1 else -1
    return k if k >= 0 else N_AA


def counts(rows):
    """AAProfileSequence of an alignment: [len][24] float32 counts."""
    rows = [rows] if isinstance(rows, str) else list(rows)
    L = len(rows[0])
    if any(len(r) != L for r in rows):
        raise ValueError("wrong alignment")
    p = np.zeros((L, N_AA + 1), np.float32)
    for r in rows:
        for i, c in enumerate(r):
            p[i, char2aa(c)] += np.float32(1.0)
    return p


def _sparse(p):
    """Per column its non-zero letters in increasing order: indices and counts,
    padded with count 0 (adding a zero product changes neither n nor v)."""
    L = p.shape[0]
    nz = p[:, :N_AA] != 0
    R = max(int(nz.sum(axis=1).max()) if L else 0, 1)
    k = np.zeros((L, R), np.int64)
    c = np.zeros((L, R), np.float32)
    for i in range(L):
        idx = np.nonzero(nz[i])[0]
        k[i, :idx.size] = idx
        c[i, :idx.size] = p[i, idx]
    return k, c


def la_score(xp, yp, table):
    """LAScore::operator() for every (i, j): [len x][len y] doubles."""
    t = np.asarray(table, np.float64).reshape(N_AA, N_AA)
    kx, cx = _sparse(xp)
    ky, cy = _sparse(yp)
    n = np.zeros((xp.shape[0], yp.shape[0]), np.float32)
    v = np.zeros((xp.shape[0], yp.shape[0]), np.float64)
    for a in range(kx.shape[1]):
        for b in range(ky.shape[1]):
            xa, yb = cx[:, a, None], cy[None, :, b]
            n = n + xa * yb                                                     # float32
            v = v + (t[kx[:, a, None], ky[None, :, b]] * xa.astype(np.float64)) * yb.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = v / n.astype(np.float64)
    return np.where(n == 0, 0.0, s)


def _exp(a):
    """libm exp, elementwise (numpy's own exp may differ in the last bit)."""
    u, inv = np.unique(a, return_inverse=True)
    out = np.empty(u.shape, np.float64)
    for i, x in enumerate(u):
        try:
            out[i] = math.exp(x)
        except OverflowError:
            out[i] = math.inf
    return out[inv].reshape(a.shape)


def _skew(s):
    """sk[d, i] = s[i-1, d-i-1] for the cells (i, j = d - i) of anti-diagonal d."""
    n, m = s.shape
    sk = np.zeros((n + m + 1, n + 1), np.float64)
    i = np.arange(1, n + 1)[:, None]
    j = np.arange(1, m + 1)[None, :]
    sk[(i + j).ravel(), np.broadcast_to(i, (n, m)).ravel()] = s.ravel()
    return sk


def kernel_profiles(xp, yp, table, gap, ext, beta, sw=False):
    """K(x, y) from the two count arrays."""
    n, m = xp.shape[0], yp.shape[0]
    if sw and (n == 0 or m == 0):
        return 0.0
    if n == 0 or m == 0:
        return 1.0
    gap, ext, beta = float(gap), float(ext), float(beta)
    s = la_score(xp, yp, table)
    D = n + m + 1
    # state[d, i] = state of cell (i, d - i); row 0 and column 0 stay zero
    M, X, Y = (np.zeros((D, n + 1)) for _ in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        if sw:
            sk = _skew(s)
            mmax = 0.0
            for d in range(2, D):
                lo, hi = max(1, d - m), min(n, d - 1)
                a, b = slice(lo, hi + 1), slice(lo - 1, hi)
                v = np.maximum(0.0, M[d - 2, b])
                v = np.maximum(v, X[d - 2, b])
                v = np.maximum(v, Y[d - 2, b])
                M[d, a] = v + sk[d, a]
                mmax = max(mmax, float(M[d, a].max()))
                X[d, a] = np.maximum(M[d - 1, b] + gap, X[d - 1, b] + ext)
                Y[d, a] = np.maximum(np.maximum(M[d - 1, a] + gap, X[d - 1, a] + gap), Y[d - 1, a] + ext)
            return mmax
        bg, be = math.exp(beta * gap), math.exp(beta * ext)
        ek = _skew(_exp(beta * s))
        X2, Y2 = np.zeros((D, n + 1)), np.zeros((D, n + 1))
        for d in range(2, D):
            lo, hi = max(1, d - m), min(n, d - 1)
            a, b = slice(lo, hi + 1), slice(lo - 1, hi)
            M[d, a] = ek[d, a] * (((1.0 + X[d - 2, b]) + Y[d - 2, b]) + M[d - 2, b])
            X[d, a] = bg * M[d - 1, b] + be * X[d - 1, b]
            Y[d, a] = bg * (M[d - 1, a] + X[d - 1, a]) + be * Y[d - 1, a]
            X2[d, a] = M[d - 1, b] + X2[d - 1, b]
            Y2[d, a] = (M[d - 1, a] + X2[d - 1, a]) + Y2[d - 1, a]
        return float(((1.0 + X2[n + m, n]) + Y2[n + m, n]) + M[n + m, n])


def kernel(x_rows, y_rows, table, gap, ext, beta, sw=False):
    """K(x, y) of two alignments (lists of rows) or sequences (strings)."""
    return kernel_profiles(counts(x_rows), counts(y_rows), table, gap, ext, beta, sw)
