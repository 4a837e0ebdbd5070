"""Generate tests/golden/stem4d_probes.npz: the long-double twin's values
(oracle/stem4d_generic.inc, rounded to double once) of the dense sets of
tests/stem4d_probes.py, which cost over a second per pair above L ~ 70.

Twin (stored):
  suite, l130, lop  x  gap 0.8 / 0.98 / 1.0 (as float32)  x  full_dp, -b 1 / 3 / 8
  col               gap 0.8, full_dp (tests/test_stem4d.py's column-kernel Gram)
  tiled             24 x 1,040 under -b 100, the three gaps (3.5 GB of planes)
Closed form only (nothing stored; tests/stem4d_probes.py evaluates it in exact
rationals at test time): every sparse probe.  The probes whose twin fits in
memory -- the seam family at |y| = 1,100 against |x| = 12 (2 GB) and the
|x| = 700 long-x probes -- are checked here against the twin once, as is every
family scaled down in tests/test_stem4d_oracle_twin.py; |x| >= 2,047 against
|y| = 40 has the closed form only.

The synthetic fold's bytes are pinned by a SHA-256 stored beside the values.

Run:  python tests/golden/make_golden_4d_probes.py      (~3 min on 8 cores)
"""
import hashlib
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import stem_kernel_amd as ska  # noqa: E402
from tests import stem4d_probes as sp  # noqa: E402


def jobs():
    out = []
    for name in sp.DENSE_SETS:
        for g in sp.DENSE_GAPS:
            for band in sp.DENSE_BANDS:
                out.append((name, g, band))
    out.append(("col", 0.8, 0))
    for g in sp.DENSE_GAPS:
        out.append(("tiled", g, sp.TILED_BAND))
    return out


def _cell(c):
    xa, xb, g, band = c
    return sp.twin(xa, xb, ska.StemKernel4D(gap=g, band=band).params)


def _probe(c):
    fam, name, g = c
    pr = next(p for p in sp.probes(fam) if p.name == name)
    return float(sp.closed_form(pr, g)), sp.twin_of_probe(pr, g), sp.probe_tol(pr)


def fold_sha():
    h = hashlib.sha256()
    for name in sp.DENSE_SETS + ("col", "tiled"):
        for s in sp.dense_set(name)[0]:
            h.update(np.ascontiguousarray(sp.folded(s), np.float64).tobytes())
    return h.hexdigest()


def main():
    cells = {}   # every distinct (x, y, gap, band) once
    for name, g, band in jobs():
        seqs, pairs = sp.dense_set(name)
        for a, b in pairs:
            cells.setdefault((seqs[a], seqs[b], g, band), len(cells))
    work = sorted(cells, key=lambda c: -(len(c[0]) * len(c[1])) ** 2)   # costly first
    with ProcessPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        vals = dict(zip(work, ex.map(_cell, work, chunksize=1)))
        checks = [(f, p.name, g) for f in ("seam", "long_x") for p in sp.probes(f) if len(p.x) <= 700
                  for g in sp.probe_gaps(p)]
        for c, (cf, tw, t) in zip(checks, ex.map(_probe, checks, chunksize=1)):
            assert abs(cf - tw) <= t * cf, (c, cf, tw, t)
            print("probe", c, "closed form", cf, "twin", tw)
    out = {}
    for name, g, band in jobs():
        seqs, pairs = sp.dense_set(name)
        out[sp.dense_key(name, g, band)] = np.array([vals[(seqs[a], seqs[b], g, band)] for a, b in pairs])
    np.savez_compressed(os.path.join(HERE, "stem4d_probes.npz"), sha=np.array(fold_sha()), **out)
    print({k: float(v.max()) for k, v in out.items()})


if __name__ == "__main__":
    main()
