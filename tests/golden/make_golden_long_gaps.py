"""Generate tests/golden/stem_long_gaps.npz: long-double oracle values of the
stem kernels at loop_gap near 1, where every edge and the length band reach
the compared digits (tests/stem_long_gaps.py).

* The class sets of L = 200, 300 and 400 (three sequences each, all ordered
  pairs) at (loop_gap, len_band) = (0.98, 0), (0.98, 10), (0.98, 30), (1.0, 0),
  (1.0, 10).
* The gap-field set: four L = 1,100 examples from caller bpp whose largest
  edge gap is 1,022, 1,023, 1,024 and 1,077, and one L = 60 sequence, all
  ordered pairs, at (0.999, 0), (0.999, 10), (0.999, 30), (1.0, 0), (1.0, 10).
* tests/test_big_dag.py::test_long_gap_edge's three pairs (big_dag.npz's
  inputs) at loop_gap 0.999 and 1.0 with the length band off: under the
  default band no node of an L <= 500 partner is matched with the pair
  (1, 1100), and the 1,077-gap edge then reaches K(x, y) in no term
  (tests/test_stem_visibility_cpu.py).

su / si: oracle/stem_dp_generic.inc in long double (orc_su_stem_ld,
orc_si_stem_ld), rounded to double once; k2 / k3: the oracle's string parts
(double).  The synthetic fold's bytes are pinned by a SHA-256 per set.  The
archive is written with fixed timestamps and no compression state that
depends on the run, so a second run gives the same bytes.

Run:  python tests/golden/make_golden_long_gaps.py      (~20 s on 8 cores)
"""
import hashlib
import io
import os
import sys
import zipfile
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import stem_kernel_amd as ska  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests import stem_long_gaps as slg  # noqa: E402

SETS = [n for n, (_, gold) in slg.CLASS_SETS.items() if gold]
BIGGAP_PAIRS = ([2, 0, 2], [2, 2, 1])  # tests/test_big_dag.py::test_long_gap_edge
_OM = {}


def _items(name):
    if name == "gap":
        return list(slg.gap_set())
    if name == "biggap":
        big = np.load(os.path.join(HERE, "big_dag.npz"))
        s = [str(v) for v in big["seqs"]]
        return [(s[0], ska.fold(s[0].lower())), (s[2], ska.fold(s[2].lower())), (str(big["gap_seq"]), big["gap_bpp"])]
    return [(s, ska.fold(s.lower())) for s in slg.class_set(name)]


def _om(name):
    if name not in _OM:
        _OM[name] = [po.OMData([s], [b], 0.01) for s, b in _items(name)]
    return _OM[name]


def _cell(args):
    name, what, g, band, i, j = args
    om = _om(name)
    ps, pi, pt = ska.SuStemKernel().params, ska.SiStemKernel().params, ska.SiStemStrKernel().params
    if what == "su":
        return po.su_stem_ld(om[i], om[j], g, ps.beta, band)
    if what == "si":
        return po.si_stem_ld(om[i], om[j], g, pi.stack, pi.covar, band)
    if what == "k2":
        return po.su_str(om[i], om[j], pt.gap, ska.SuStemStrKernel().params.alpha)
    return po.si_str(om[i], om[j], pt.gap, pt.match, pt.mismatch)


def _write(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    arrays = {}
    with ProcessPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        def matrix(name, what, g, band, n):
            cells = [(name, what, g, band, i, j) for i in range(n) for j in range(n)]
            return np.array(list(ex.map(_cell, cells, chunksize=1))).reshape(n, n)
        for name in SETS + ["gap"]:
            items = _items(name)
            n = len(items)
            arrays[f"{name}_seqs"] = np.array([s for s, _ in items])
            if name != "gap":
                h = hashlib.sha256()
                for _, b in items:
                    h.update(np.ascontiguousarray(b, np.float64).tobytes())
                arrays[f"{name}_sha"] = np.array(h.hexdigest())
            for what in ("k2", "k3"):
                arrays[f"{name}_{what}"] = matrix(name, what, 0.0, 0, n)
            for g, band in (slg.GAP_PARAMS if name == "gap" else slg.PARAMS):
                for what in ("su", "si"):
                    arrays[slg._key(name, g, band, what)] = matrix(name, what, g, band, n)
                print(name, g, band, flush=True)
        for g in (0.999, 1.0):
            for kind, what in ((0, "su"), (1, "si")):
                cells = [("biggap", what, g, 0, i, j) for i, j in zip(*BIGGAP_PAIRS)]
                arrays[f"biggap_g{g}_b0_K{kind}"] = np.array(list(ex.map(_cell, cells, chunksize=1)))
    _write(os.path.join(HERE, "stem_long_gaps.npz"), arrays)


if __name__ == "__main__":
    main()
