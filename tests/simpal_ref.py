"""Restatement of the reference's simple palindrome kernel (a helper, not a
test file): Pals::make_pal_map and KernelFunc::operator() of simpal/simpal.cpp.

entries()      the map of one sequence, float32 arithmetic, same-(key, d)
               weights added in the project's defined order (increasing i, then
               increasing r); the reference adds them in the iteration order
               of a hash_multimap, which a two-term sum does not depend on.
kernel_seq()   the double loop of KernelFunc in map order with math.exp.
kernel_vec()   the same sum vectorised (numpy) for large cases; its summation
               order differs, so it agrees to rounding, not bit for bit.
"""
import math

import numpy as np

_COMP = {"a": "u", "c": "g", "g": "c", "u": "a", "t": "a"}
_CODE = {"a": 0, "c": 1, "g": 2, "u": 3}


def tri(n, i, j):
    """Index of p(i, j), 0-based i < j, in the packed strict upper triangle."""
    return i * n - i * (i + 1) // 2 + (j - i - 1)


def entries(seq, bpp, seed_length=3, min_loop=3, max_dist=300, with_multiplicity=False):
    """(keys, dist, weight) in map order (key, then dist); with_multiplicity
    adds the largest number of weights summed into one entry."""
    seq = seq.lower()  # load_examples, simpal.cpp:298
    n, s = len(seq), seed_length
    if n < s:
        raise ValueError("sequence shorter than seed_length")
    bpp = np.asarray(bpp, dtype=np.float64)
    rev = "".join(_COMP.get(c, "\0") for c in reversed(seq))  # RevComp, :73-95
    rpos = {}
    for r in range(n - s):  # the last k-mer is skipped, :116
        rpos.setdefault(rev[r:r + s], []).append(r)
    pals, mult = {}, {}
    for i in range(n - s):
        k = seq[i:i + s]
        for r in rpos.get(k, ()):
            d = n - i - r - 2 * s  # unsigned in the reference (:152): negative fails
            if d < 0 or d < min_loop or d > max_dist:
                continue
            w = np.float32(1.0)
            for t in range(s):  # pf(m, n) as float, product in float (:156-203)
                w = np.float32(bpp[tri(n, i + t, n - r - t - 1)]) * w
            if (k, d) in pals:
                pals[(k, d)] = np.float32(pals[(k, d)] + w)
                mult[(k, d)] += 1
            else:
                pals[(k, d)] = w
                mult[(k, d)] = 1
    order = sorted(pals)
    keys = [k for k, _ in order]
    dist = np.array([d for _, d in order], dtype=np.int32)
    w = np.array([pals[e] for e in order], dtype=np.float32)
    if with_multiplicity:
        return keys, dist, w, max(mult.values(), default=0)
    return keys, dist, w


def mismatches(a, b):
    return sum(1 for x, y in zip(a, b) if x != y)


def kernel_seq(A, B, tolerance=1):
    """KernelFunc::operator() (simpal.cpp:236-266): a outer, b inner, both in
    map order, each term (exp(-dist) * w_a) * w_b in double."""
    ka, da, wa = A
    kb, db, wb = B
    ret = 0.0
    for i in range(len(ka)):
        for j in range(len(kb)):
            if tolerance < 0 or mismatches(ka[i], kb[j]) <= tolerance:
                dist = abs(int(da[i]) - int(db[j]))
                ret += (math.exp(-dist) * float(wa[i])) * float(wb[j])
    return ret


def _codes(keys):
    if not keys:
        return np.zeros((0, 1), np.int8)
    return np.array([[_CODE[c] for c in k] for k in keys], dtype=np.int8)


def kernel_vec(A, B, tolerance=1, chunk=512):
    """The same sum with numpy, x entries in chunks."""
    ka, da, wa = A
    kb, db, wb = B
    if len(ka) == 0 or len(kb) == 0:
        return 0.0
    ca, cb = _codes(ka), _codes(kb)
    da = np.asarray(da, np.int64)
    db = np.asarray(db, np.int64)
    wa = np.asarray(wa, np.float64)
    wb = np.asarray(wb, np.float64)
    total = 0.0
    for a0 in range(0, len(ka), chunk):
        a1 = min(a0 + chunk, len(ka))
        with np.errstate(under="ignore"):
            e = np.exp(-np.abs(da[a0:a1, None] - db[None, :]).astype(np.float64))
        t = (e * wa[a0:a1, None]) * wb[None, :]
        if tolerance >= 0:
            mm = (ca[a0:a1, None, :] != cb[None, :, :]).sum(axis=2)
            t = np.where(mm <= tolerance, t, 0.0)
        total += float(t.sum())
    return total


def gram(examples, tolerance=1, normalize=False, kernel=kernel_vec):
    """The Gram of a list of (keys, dist, weight); normalize: the reference's
    -n (common/kernel_matrix.cpp:560-571), K_ij / sqrt(K_ii K_jj) off the
    diagonal -- NaN in the row and column of a zero diagonal -- and the
    diagonal set to 1."""
    n = len(examples)
    K = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            K[i, j] = K[j, i] = kernel(examples[i], examples[j], tolerance)
    if normalize:
        d = np.sqrt(np.diag(K).copy())
        with np.errstate(invalid="ignore", divide="ignore"):
            K = K / (d[:, None] * d[None, :])
        np.fill_diagonal(K, 1.0)
    return K
