"""CPU check of the string fast path's streamed schedule (profile_string.hip:
str_fast_pair and the boundary initialisation of sk_str_fast_kernel),
emulated in numpy lane by lane: windows (lane w starts its next row) and
interiors, Lys = max(Ly, 64), the step count T, the wrap (xr = xn, dG = dn,
yofs = 0), lane 63's LDS boundary writes, the operands and column-0 power
fetched for the next strip, and the owner lane.  The DP must equal the
oracle's over a grid of lengths around 1, 63-66, 127-130 and 191-193, and
two deliberate faults -- dn read one power off, the row-0 boundary zeroed
from column 64 -- must fail it (tests/test_bpla_schedule.py covers the
unstreamed schedule the kernel started from)."""
import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests import string_long_gaps as sg
from tests.helpers import make_examples

LENGTHS = (1, 2, 5, 40, 63, 64, 65, 66, 100, 127, 128, 129, 130, 191, 192, 193)
CODE = {c: k for k, c in enumerate("ACGU")}


def _factors(x, y, match, mismatch):
    cx, cy = np.array([CODE[c] for c in x]), np.array([CODE[c] for c in y])
    return np.where(cx[:, None] == cy[None, :], match, mismatch).astype(np.float64)


def _shr1(v, b):
    """DPP wave_shr: lane k gets lane k - 1's value, lane 0 gets b."""
    out = np.empty(64)
    out[1:] = v[:-1]
    out[0] = b
    return out


def fast_pair(F, gap, dn_off=0, zero_row0_from=None):
    """K0[Lx][Ly] by the kernel's schedule; F[i][j] the cell factors.
    dn_off: read the next strip's column-0 power that far off (a fault);
    zero_row0_from: initialise G0[0][j] to 0 from that column on (a fault)."""
    Lx, Ly = F.shape
    if Lx == 0 or Ly == 0:
        return 1.0
    gpow = sg.gap_powers(gap, max(Lx, Ly, 60) + 4)  # the host's table: 64 powers at least
    lane = np.arange(64)
    Lys = max(Ly, 64)
    # sk_str_fast_kernel: row 0 into the boundary row
    bnd = np.zeros((Lys + 2, 2))
    for j in range(Lys + 1):
        bnd[j, 0] = 1.0
        bnd[j, 1] = gpow[j] if j <= Ly else 0.0
        if zero_row0_from is not None and j >= zero_row0_from:
            bnd[j, 1] = 0.0
    nstrips = (Lx + 63) // 64
    T = (nstrips - 1) * Lys + ((Lx - 1) & 63) + Ly
    xn = np.minimum(lane, Lx - 1)
    dn = gpow[lane]
    xr = xn.copy()
    yofs = np.zeros(64, dtype=np.int64)
    lK1, lG1, lK0, lG0, dG = (np.zeros(64) for _ in range(5))

    def cell(uK, uG, c1, on):
        nonlocal lK1, lG1, lK0, lG0
        f = F[xr, np.minimum(yofs, Ly - 1)]  # (lanes that are off read past the row: unused)
        v = dG * f
        K1 = np.where(c1, v, v + lK1)
        G1 = np.where(c1, v, lG1 * gap + v)
        lK1, lG1 = np.where(on, K1, lK1), np.where(on, G1, lG1)
        lK0, lG0 = np.where(on, K1 + uK, lK0), np.where(on, uG * gap + G1, lG0)

    all_on = np.ones(64, dtype=bool)
    no = np.zeros(64, dtype=bool)
    for s in range(nstrips + 1):
        Ws = s * Lys
        wend = min(64, T - Ws)
        if wend <= 0:
            break
        for w in range(wend):  # window step w of strip s
            wrap = lane == w
            xr = np.where(wrap, xn, xr)
            dG = np.where(wrap, dn, dG)
            yofs = np.where(wrap, 0, yofs)
            jl = np.where(lane <= w, w - lane + 1, Lys + w - lane + 1)
            on = (jl <= Ly) & np.where(lane <= w, s < nstrips, s > 0)
            jb = w + 1
            bj = bnd[jb if jb <= Ly else 0].copy()
            uK, uG = _shr1(lK0, bj[0]), _shr1(lG0, bj[1])
            cell(uK, uG, wrap, on)
            if on[63]:
                bnd[jl[63]] = (lK0[63], lG0[63])
            dG = uG
            yofs = yofs + 1
        if s + 1 < nstrips:
            i1 = 64 * (s + 1) + lane
            xn = np.minimum(i1, Lx - 1)
            dn = gpow[np.clip(np.minimum(i1, Lx) + dn_off, 0, len(gpow) - 1)]
        tend = min(Ws + Lys, T) if s < nstrips else 0
        for t in range(Ws + 64, tend):  # interior: lane 0 at column jb
            jb = t - Ws + 1
            bj = bnd[jb].copy()
            uK, uG = _shr1(lK0, bj[0]), _shr1(lG0, bj[1])
            cell(uK, uG, no, all_on)
            bnd[jb - 63] = (lK0[63], lG0[63])
            dG = uG
            yofs = yofs + 1
    return float(lK0[(Lx - 1) & 63])


@pytest.mark.parametrize("gap", [0.8, 1.0])
def test_schedule_matches_oracle_on_the_length_grid(gap):
    a, b = ska.random_sequences(2, max(LENGTHS), 0x5EED0D00)
    match, mismatch = 1.0, 0.8
    worst = 0.0
    oms = {}
    for L in LENGTHS:
        oms[L] = make_examples([a[:L], b[-L:]], use_bp=False)[1]
    for lx in LENGTHS:
        for ly in LENGTHS:
            got = fast_pair(_factors(a[:lx], b[-ly:], match, mismatch), gap)
            ref = po.si_str_ld(oms[lx][0], oms[ly][1], gap, match, mismatch)
            err = abs(got - ref) / ref
            worst = max(worst, err / (sg.rounding_depth(lx, ly, "onehot") * sg.U))
            assert err <= sg.rounding_depth(lx, ly, "onehot") * sg.U, (lx, ly, got, ref)
    print(f"gap {gap}: schedule against the _ld twin, worst error / (D 2^-53) {worst:.3g}")


def _probe_case(lx, i, ly, j):
    x, y = sg.probe(lx, (i,), "A"), sg.probe(ly, (j,), "U")
    return _factors(x, y, 1.0, 0.0), i, j


# (Lx, i, Ly, j): a probe in column 1 below every strip boundary, in row 1 beyond column 63, and both with Ly < 64
PROBES = [(193, 65, 200, 1), (193, 129, 5, 1), (193, 193, 200, 1), (129, 128, 64, 1), (1, 1, 200, 65), (1, 1, 200, 200),
          (65, 1, 129, 128), (193, 129, 200, 129), (65, 65, 5, 5), (130, 66, 63, 63)]


@pytest.mark.parametrize("gap", [0.98, 0.999])
def test_schedule_on_probes_and_its_teeth(gap):
    gp = sg.gap_powers(gap, 400)
    caught = {"dn": 0, "row0": 0}
    for lx, i, ly, j in PROBES:
        F, _, _ = _probe_case(lx, i, ly, j)
        want = 1.0 + gp[i + j - 2]
        tol = sg.rounding_depth(lx, ly, "onehot") * sg.U
        assert abs(fast_pair(F, gap) - want) <= tol * want, (lx, i, ly, j)
        # the faults: wherever a case reads the faulty value it must miss by far more than the tolerance
        if j == 1 and i > 64:
            bad = fast_pair(F, gap, dn_off=-1)
            assert abs(bad - want) > 100 * tol * want, (lx, i, ly, j, bad, want)
            caught["dn"] += 1
        if i == 1 and j > 64:
            bad = fast_pair(F, gap, zero_row0_from=64)
            assert abs(bad - want) > 100 * tol * want, (lx, i, ly, j, bad, want)
            caught["row0"] += 1
    assert caught["row0"] >= 3 and caught["dn"] >= 3   # (at gap 1 every power is 1: the grid test covers it)


def test_dense_inputs_do_not_see_the_faults():
    """Why the probes exist: on random sequences even at gap 1 both faults
    stay below the derived tolerance (printed: error / tolerance)."""
    a, b = ska.random_sequences(2, 193, 0x5EED0D01)
    F = _factors(a, b, 1.0, 0.8)
    good = fast_pair(F, 0.98)
    tol = sg.str_tol(193, 193, "onehot")
    for what, bad in (("dn one power off", fast_pair(F, 0.98, dn_off=-1)),
                      ("row 0 zeroed from column 64", fast_pair(F, 0.98, zero_row0_from=64))):
        print(f"random L = 193, gap 0.98, {what}: change / tolerance {abs(bad - good) / good / tol:.3g}")
