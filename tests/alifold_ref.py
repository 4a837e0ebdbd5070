"""Reference restatements of the consensus (alifold-style) fold's model
(sk_fold_alignment), for the tests only, in plain Python/numpy:

(a) ``enumerate_alignment``: the Boltzmann sum over EVERY consensus structure,
    each row's energy taken loop by loop from the engine's loop model
    (csrc/host/fold_params.h) -- exponential, short alignments only;
(b) ``fold_alignment_dp``: an inside-outside DP of the same model for the
    lengths (a) cannot reach.  (b) is pinned by (a) in test_alifold.py.

Model.  S rows of n columns; A C G U T (any case, T = U) are letters, every
other character is blank.  Per-row type of columns (i, j): 7 if both blank,
else the engine's pair type (CG1 GC2 UG3 GU4 AU5 UA6 by letters; GU/UG -> 0
under no_gu), 0 = no pair.  With pf[t] the rows of type t,
    score  = sum_{1<=k<l<=6} pf[k] pf[l] Hamming(letters of k, letters of l)
    pscore = (100 score) // S - 100 pf[0] - 25 pf[7]
and (i, j) may pair iff j - i >= 4, 2 pf[0] <= S, pscore >= -200 (and it
survives the lonely-pair walk under no_lonely_pairs).  A structure weighs
    exp(-(sum_s E_s - sum_pairs pscore) / (S kT)),
E_s the single-sequence loop energies on row s with loop sizes in columns,
type 0 read as 7: no stacking energy with a type 7 on either side, terminal
penalty paid (7 > 2).
"""
import math

import numpy as np

KT = (37.0 + 273.15) * 1.98717 / 10.0
LXC = 107.856
STACK = [[0, 0, 0, 0, 0, 0, 0],
         [0, -240, -330, -210, -140, -210, -210],
         [0, -330, -340, -250, -150, -220, -240],
         [0, -210, -250, 130, -50, -140, -130],
         [0, -140, -150, -50, 30, -60, -100],
         [0, -210, -220, -140, -60, -110, -90],
         [0, -210, -240, -130, -100, -90, -130]]
HAIRPIN = [0, 0, 0, 570, 560, 560, 540, 590, 560, 640, 650, 660, 670, 678, 686, 694, 701, 707, 713, 719,
           725, 730, 735, 740, 744, 749, 753, 757, 761, 765, 769]
BULGE = [0, 380, 280, 320, 360, 400, 440, 459, 470, 480, 490, 500, 510, 519, 527, 534, 541, 548, 554, 560,
         565, 571, 576, 580, 585, 589, 594, 598, 602, 605, 609]
INTERIOR = [0, 0, 410, 510, 170, 180, 200, 220, 230, 240, 250, 260, 270, 278, 286, 294, 301, 307, 313, 319,
            325, 330, 335, 340, 345, 349, 353, 357, 361, 365, 369]
ML_CLOSING, ML_INTERN, TERMINAL_AU, NINIO, MAX_NINIO, MAXLOOP = 340, 40, 50, 50, 300, 30

# the engine's pair-type table by codes A0 C1 G2 U3 (fold_dev.h kFoldPairBits, oracle/fold_oracle.c pair_type)
PAIR = [[0, 0, 0, 5], [0, 0, 1, 0], [0, 2, 0, 4], [6, 0, 3, 0]]
LETTERS = {PAIR[a][b]: (a, b) for a in range(4) for b in range(4) if PAIR[a][b]}


def code(ch):
    return {"A": 0, "C": 1, "G": 2, "U": 3, "T": 3}.get(ch.upper(), -1)


def hamming(k, l):
    return (LETTERS[k][0] != LETTERS[l][0]) + (LETTERS[k][1] != LETTERS[l][1])


def row_type(a, b, no_gu):
    if a < 0 and b < 0:
        return 7
    if a < 0 or b < 0:
        return 0
    t = PAIR[a][b]
    return 0 if no_gu and t in (3, 4) else t


def pscore_of(pf, S):
    score = sum(pf[k] * pf[l] * hamming(k, l) for k in range(1, 7) for l in range(k + 1, 7))
    return (100 * score) // S - 100 * pf[0] - 25 * pf[7]


class Model:
    """Codes, per-row types, pscores and the allowed column pairs of one alignment."""

    def __init__(self, rows, no_gu=False, no_lonely_pairs=False):
        self.S, self.n = len(rows), len(rows[0])
        assert self.S >= 1 and all(len(r) == self.n for r in rows)
        S, n = self.S, self.n
        self.T = S * KT
        self.c = [[code(ch) for ch in r] for r in rows]
        self.no_gu = no_gu
        self.pscore = np.zeros((n, n), dtype=np.int64)
        self.allowed = np.zeros((n, n), dtype=bool)
        for i in range(n):
            for j in range(i + 1, n):
                pf = [0] * 8
                for c in self.c:
                    pf[row_type(c[i], c[j], no_gu)] += 1
                ps = pscore_of(pf, S)
                self.pscore[i, j] = ps
                self.allowed[i, j] = j - i >= 4 and 2 * pf[0] <= S and ps >= -200
        if no_lonely_pairs:
            self.allowed = self._lonely(self.allowed)

    def _lonely(self, can):
        """The legacy pair-type filter's walk (oracle/fold_oracle.c lonely_filter) over `can`."""
        n = self.n
        lp = np.zeros((n, n), dtype=bool)
        for k in range(n):
            for l in (1, 2):
                i, j = k, k + 3 + l
                if j >= n:
                    continue
                otype, ntype, typ = False, False, bool(can[i, j])
                while i >= 0 and j < n:
                    if i > 0 and j < n - 1:
                        ntype = bool(can[i - 1, j + 1])
                    if not otype and not ntype:
                        typ = False
                    lp[i, j] = typ
                    otype, typ = typ, ntype
                    i -= 1
                    j += 1
        return lp

    # ---- per-row loop energies (dcal/mol), type 0 read as 7
    def etype(self, s, i, j):
        t = row_type(self.c[s][i], self.c[s][j], self.no_gu)
        return t if t else 7

    def rtype(self, s, p, q):
        """the inner pair (p, q) read from its other side, as a stack does"""
        e = self.etype(s, p, q)
        return 7 if e == 7 else PAIR[self.c[s][q]][self.c[s][p]]

    @staticmethod
    def au(e):
        return TERMINAL_AU if e > 2 else 0

    @staticmethod
    def stack(e1, e2):
        return 0 if e1 == 7 or e2 == 7 else STACK[e1][e2]

    def e_hairpin(self, s, i, j):
        u = j - i - 1
        e = HAIRPIN[min(u, 30)] + (LXC * math.log(u / 30.0) if u > 30 else 0.0)
        return e + self.au(self.etype(s, i, j))

    def e_interior(self, s, i, j, p, q):
        e1, e2 = self.etype(s, i, j), self.rtype(s, p, q)
        n1, n2 = p - i - 1, j - q - 1
        u = n1 + n2
        if u == 0:
            return self.stack(e1, e2)
        if n1 == 0 or n2 == 0:
            return BULGE[u] + (self.stack(e1, e2) if u == 1 else self.au(e1) + self.au(e2))
        return INTERIOR[u] + min(MAX_NINIO, NINIO * abs(n1 - n2)) + self.au(e1) + self.au(e2)

    def structure_energy(self, pt):
        """sum over the rows of the energy of structure pt (partner or -1), minus the pscores;
        None when a loop is not formed (an interior loop over MAXLOOP)."""
        n, tot = self.n, 0.0
        for i in range(n):
            j = pt[i]
            if j <= i:
                continue
            tot -= float(self.pscore[i, j])
            br, k = [], i + 1
            while k < j:
                if pt[k] > k:
                    br.append((k, pt[k]))
                    k = pt[k]
                k += 1
            for s in range(self.S):
                if not br:
                    tot += self.e_hairpin(s, i, j)
                elif len(br) == 1:
                    p, q = br[0]
                    if (p - i - 1) + (j - q - 1) > MAXLOOP:
                        return None
                    tot += self.e_interior(s, i, j, p, q)
                else:
                    tot += ML_CLOSING + ML_INTERN + self.au(self.etype(s, i, j))
                    tot += sum(ML_INTERN + self.au(self.etype(s, p, q)) for p, q in br)
        k = 0
        while k < n:
            if pt[k] > k:
                tot += sum(self.au(self.etype(s, k, pt[k])) for s in range(self.S))
                k = pt[k]
            k += 1
        return tot


def tri(n, i, j):
    return i * n - i * (i + 1) // 2 + (j - i - 1)


def enumerate_alignment(rows, no_gu=False, no_lonely_pairs=False):
    """(ln Z, packed probabilities, number of structures, Model) by exhaustive enumeration."""
    M = Model(rows, no_gu, no_lonely_pairs)
    n = M.n
    pt = [-1] * n
    acc = {"Z": 0.0, "count": 0}
    bpp = np.zeros(n * (n - 1) // 2 if n > 1 else 0)

    def rec(i):
        while i < n and pt[i] >= 0:
            i += 1
        if i >= n:
            e = M.structure_energy(pt)
            if e is not None:
                w = math.exp(-e / M.T)
                acc["Z"] += w
                acc["count"] += 1
                for a in range(n):
                    if pt[a] > a:
                        bpp[tri(n, a, pt[a])] += w
            return
        rec(i + 1)
        lim = n
        for k in range(i - 1, -1, -1):
            if pt[k] > i:
                lim = pt[k]
                break
        for j in range(i + 4, lim):
            if M.allowed[i, j]:
                pt[i], pt[j] = j, i
                rec(i + 1)
                pt[i] = pt[j] = -1

    rec(0)
    return math.log(acc["Z"]), bpp / acc["Z"], acc["count"], M


def fold_alignment_dp(rows, no_gu=False, no_lonely_pairs=False):
    """(ln Z, packed probabilities) by McCaskill's inside-outside recursions over
    Qb, Qm1, Qm and Q5, the loop energies summed over the rows in numpy tables."""
    M = Model(rows, no_gu, no_lonely_pairs)
    S, n, T = M.S, M.n, M.T
    if n < 5:
        return 0.0, np.zeros(n * (n - 1) // 2 if n > 1 else 0)
    c = np.array(M.c)                                            # S x n
    both = (c[:, :, None] < 0) & (c[:, None, :] < 0)
    ptab = np.array(PAIR)
    raw = np.where((c[:, :, None] < 0) | (c[:, None, :] < 0), 0, ptab[np.maximum(c[:, :, None], 0),
                                                                      np.maximum(c[:, None, :], 0)])
    if no_gu:
        raw = np.where((raw == 3) | (raw == 4), 0, raw)
    et = np.where(both | (raw == 0), 7, raw)                    # energy type of (i, j), S x n x n
    rt = np.where(et == 7, 7, np.transpose(np.where(raw == 0, 7, raw), (0, 2, 1)))  # (p, q) read as (q, p)
    m = (et > 2).sum(0).astype(float)                            # rows paying the terminal penalty
    st8 = np.zeros((8, 8))
    st8[1:7, 1:7] = np.array(STACK)[1:, 1:]
    St0, St1, St2 = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    St0[:-1, 1:] = st8[et[:, :-1, 1:], rt[:, 1:, :-1]].sum(0)   # inner (i+1, j-1)
    St1[:-2, 1:] = st8[et[:, :-2, 1:], rt[:, 2:, :-1]].sum(0)   # inner (i+2, j-1)
    St2[:-1, 2:] = st8[et[:, :-1, 2:], rt[:, 1:, :-2]].sum(0)   # inner (i+1, j-2)
    C = np.where(M.allowed, np.exp(M.pscore / T), 0.0)
    A = np.exp(-m * TERMINAL_AU / T)

    def bz(e):  # Boltzmann factor of an energy every row pays
        return math.exp(-e / KT)

    hp = np.zeros(n + 1)
    for u in range(3, n + 1):
        hp[u] = bz(HAIRPIN[min(u, 30)] + (LXC * math.log(u / 30.0) if u > 30 else 0.0))
    # loops (n1, n2), n1 + n2 <= MAXLOOP, and the part of their energy every row shares
    N1, N2 = np.array([(a, b) for a in range(MAXLOOP + 1) for b in range(MAXLOOP + 1 - a)]).T
    U = N1 + N2
    shared = np.array([0.0 if u == 0 else BULGE[u] if (a == 0 or b == 0) else
                       INTERIOR[u] + min(MAX_NINIO, NINIO * abs(a - b)) for a, b, u in zip(N1, N2, U)])
    fsh = np.exp(-shared / KT)
    k_stack = int(np.where((N1 == 0) & (N2 == 0))[0][0])
    k_b1 = int(np.where((N1 == 1) & (N2 == 0))[0][0])
    k_b2 = int(np.where((N1 == 0) & (N2 == 1))[0][0])
    mlc, mli = bz(ML_CLOSING + ML_INTERN), bz(ML_INTERN)

    def loop_w(i, j, P, Q, ok):
        """weights of the loops (i, j) -> (P, Q): cells x loops"""
        Pc, Qc = np.where(ok, P, 0), np.where(ok, Q, 0)
        w = fsh[None, :] * A[i, j][:, None] * A[Pc, Qc]
        w[:, k_stack] = np.exp(-St0[i, j] / T)
        w[:, k_b1] = fsh[k_b1] * np.exp(-St1[i, j] / T)
        w[:, k_b2] = fsh[k_b2] * np.exp(-St2[i, j] / T)
        return np.where(ok, w, 0.0)

    Qb, Qm, Qm1 = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    for d in range(4, n):
        i = np.arange(n - d)
        j = i + d
        P, Q = i[:, None] + 1 + N1[None, :], j[:, None] - 1 - N2[None, :]
        ok = Q - P >= 4
        inner = (np.where(ok, Qb[np.where(ok, P, 0), np.where(ok, Q, 0)], 0.0) * loop_w(i, j, P, Q, ok)).sum(1)
        ci, cj = i[:, None], j[:, None]
        E = np.arange(5, d - 5)[None, :]  # u = i + e, u + 5 <= j - 1
        ml = (Qm[ci + 1, ci + E] * Qm1[ci + E + 1, cj - 1]).sum(1)
        Qb[i, j] = C[i, j] * (hp[d - 1] * A[i, j] + inner + ml * mlc * A[i, j])
        Qm1[i, j] = Qm1[i, j - 1] + Qb[i, j] * mli * A[i, j]
        E = np.arange(0, d - 3)[None, :]  # u = i + e, u + 4 <= j; Qm(i, i - 1) = 0 at e = 0
        mm = ((1.0 + np.where(E >= 1, Qm[ci, np.maximum(ci + E - 1, 0)], 0.0)) * Qm1[ci + E, cj]).sum(1)
        Qm[i, j] = mm
    ext = Qb * A
    Q5 = np.zeros(n + 1)
    Q5[0] = 1.0
    for j in range(n):
        Q5[j + 1] = Q5[j] + (Q5[:max(j - 3, 0)] * ext[:max(j - 3, 0), j]).sum()
    Z = Q5[n]
    H5 = np.zeros(n + 2)
    H5[n] = 1.0
    for k in range(n - 1, -1, -1):
        H5[k] = H5[k + 1] + (H5[k + 5:n + 1] * ext[k, k + 4:n]).sum()
    # outside: Hb = dZ/dQb, Hx = Hb C (the adjoint of the bracket), each cell pulling from larger spans
    Hb, Hx, Hm, Hm1 = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    for d in range(n - 1, 3, -1):
        i = np.arange(n - d)
        j = i + d
        ci, cj = i[:, None], j[:, None]
        # Hm(i, j).  Qm(i, j2) = .. + Qm(i, j) Qm1(j + 1, j2), j2 >= j + 5
        J2 = cj + np.arange(5, max(n - d, 5))[None, :]
        v = J2 < n
        J2 = np.where(v, J2, 0)
        hm = np.where(v, Hm[ci, J2] * Qm1[np.minimum(cj + 1, n - 1), J2], 0.0).sum(1)
        # closing pair (i - 1, jp), jp >= j + 6: its multiloop splits into Qm(i, j) Qm1(j + 1, jp - 1)
        JP = cj + np.arange(6, max(n - d, 6))[None, :]
        v = (JP < n) & (ci >= 1)
        JP, IP = np.where(v, JP, 1), np.where(v, ci - 1, 0)
        hm += np.where(v, Hx[IP, JP] * mlc * A[IP, JP] * Qm1[np.minimum(cj + 1, n - 1), JP - 1], 0.0).sum(1)
        Hm[i, j] = hm
        # Hm1(i, j).  Qm(ii, j) = .. + (1 + Qm(ii, i - 1)) Qm1(i, j), ii = i - e
        E = np.arange(0, n - d)[None, :]
        v = ci - E >= 0
        II = np.where(v, ci - E, 0)
        hm1 = np.where(v, Hm[II, cj] * (1.0 + np.where(E >= 1, Qm[II, np.maximum(ci - 1, 0)], 0.0)), 0.0).sum(1)
        # closing pair (i - e, j + 1), e >= 6: Qm(i - e + 1, i - 1) Qm1(i, j)
        E = np.arange(6, max(n - d, 6))[None, :]
        v = (ci - E >= 0) & (cj + 1 < n)
        IP, JP = np.where(v, ci - E, 0), np.where(v, cj + 1, 0)
        hm1 += np.where(v, Hx[IP, JP] * mlc * A[IP, JP] * Qm[np.minimum(IP + 1, n - 1), np.maximum(ci - 1, 0)],
                        0.0).sum(1)
        Hm1[i, j] = hm1
        # branch of a multiloop: Qm1(i, jj) for jj >= j (the row's shorter spans are still zero)
        hb = Hm1[:n - d].sum(1) * mli * A[i, j]
        hb += H5[j + 1] * Q5[i] * A[i, j]
        # enclosing loops (ip, jp) = (i - 1 - n1, j + 1 + n2)
        IP, JP = i[:, None] - 1 - N1[None, :], j[:, None] + 1 + N2[None, :]
        ok = (IP >= 0) & (JP < n)
        IPc, JPc = np.where(ok, IP, 0), np.where(ok, JP, 0)
        w = fsh[None, :] * A[IPc, JPc] * A[i, j][:, None]
        w[:, k_stack] = np.exp(-St0[IPc[:, k_stack], JPc[:, k_stack]] / T)
        w[:, k_b1] = fsh[k_b1] * np.exp(-St1[IPc[:, k_b1], JPc[:, k_b1]] / T)
        w[:, k_b2] = fsh[k_b2] * np.exp(-St2[IPc[:, k_b2], JPc[:, k_b2]] / T)
        hb += (np.where(ok, Hx[IPc, JPc] * w, 0.0)).sum(1)
        Hb[i, j] = hb
        Hx[i, j] = hb * C[i, j]
    P = Qb * Hb / Z
    return math.log(Z), P[np.triu_indices(n, 1)]
