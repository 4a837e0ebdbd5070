"""The DAG stem kernel on y's numbered by the renumbering pass (host/pack_sweep.cpp
renumber_equal_lengths; the packed arrays themselves:
tests/test_y_renumber_cpu.py).  Every ordered pair of each set is computed

  - on the default pack, against the C oracle at 1e-6 relative (the tolerance
    of tests/test_gamma.py), and
  - on the experiments build also on the pack in the plain stable order
    (SK_NO_Y_RENUMBER=1, read when a dataset is packed): against the oracle at
    1e-6, and against the default pack at 1e-12 relative, the bound the
    project uses between schedules (tests/test_shared_sums.py) -- the order
    of the y nodes changes only the association of the sums over them --
    with the shared Gamma / Phi tables and with the per-item path forced
    (SK_GAM_TABLE_MB=0, SK_PHI_TABLE_MB=0).

Sets: 24 sequences at L = 40 (runs of many equal-length nodes, the narrow
register classes); 24 at L = 200 from the benchmark's seed plus the two
MAXK 20 sequences of the config-size fixtures (register classes 16, 17 and
20; the oracle on two x per y, 52 pairs, the other pairs between the packs
only); and gapped three-row alignments among single sequences, whose y's run
the full schedule.  Every test asserts through sk_dataset_sweep_conflicts
which numbering its dataset holds.  LSuStemStrKernel runs once on the L = 40
set, so that the string kernel rides along."""
import os

import numpy as np
import pytest

import stem_kernel_amd as ska
from oracle import pyoracle as po
from tests.helpers import make_examples, mutate_alignment, rel_err

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 0x5EED0002
KNOBS = ("SK_NO_Y_RENUMBER", "SK_GAM_TABLE_MB", "SK_PHI_TABLE_MB")


def _items(name):
    if name == "L40":
        return ska.random_sequences(24, 40, SEED + 40), ska.SuStemKernel(loop_gap=0.4)
    if name == "L200":
        dag = np.load(os.path.join(GOLDEN, "large_dag.npz"))
        return ska.random_sequences(24, 200, SEED) + [str(s) for s in dag["ns20_L200_seqs"]], ska.SuStemKernel()
    base = ska.random_sequences(10, 64, SEED + 64)
    return ([mutate_alignment(s, 3, SEED + k) for k, s in enumerate(base[:6])] + base[6:8] +
            [mutate_alignment(s, 2, SEED + 8 + k, gap=0.0) for k, s in enumerate(base[8:])],
            ska.SuStemKernel(loop_gap=0.4, len_band=4))


def _sample(name, n):
    """the pairs the oracle computes: all, or at L = 200 two x per y"""
    if name != "L200":
        return [(i, j) for i in range(n) for j in range(n)]
    return [((j + d) % n, j) for j in range(n) for d in (1, 7)]


class _Case:
    def __init__(self, name):
        self.name = name
        self.items, self.kern = _items(name)
        self.n = len(self.items)
        _, om = make_examples(self.items)
        p = self.kern.params
        self.sample = _sample(name, self.n)
        self.ref = np.array([po.su_stem(om[i], om[j], p.loop_gap, p.beta, p.len_band) for i, j in self.sample])

    def pairs(self, ctx, plain=False, per_item=False):
        """(all ordered pairs as an n x n matrix, the dataset), the dataset packed and run with the switches set"""
        saved = {k: os.environ.pop(k, None) for k in KNOBS}
        try:
            if plain:
                os.environ["SK_NO_Y_RENUMBER"] = "1"
            if per_item:
                os.environ["SK_GAM_TABLE_MB"] = os.environ["SK_PHI_TABLE_MB"] = "0"
            ds, _ = make_examples(self.items)
            x, y = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(self.n), np.arange(self.n), indexing="ij"))
            got = ctx.pairs(ds, self.kern, x, y).reshape(self.n, self.n)
            shared = ctx.last_gamma_shared()
            return got, ds, shared
        finally:
            for k in KNOBS:
                os.environ.pop(k, None)
                if saved[k] is not None:
                    os.environ[k] = saved[k]

    def oracle_err(self, got):
        return rel_err(np.array([got[i, j] for i, j in self.sample]), self.ref)

    def numbering(self, ds):
        """(model cycles of the packed sweep chunks, of the packer's numbering, of the plain order) over the set"""
        packed = new = plain = 0
        for i in range(self.n):
            c, y = ds.sweep_conflicts(i), ds.y_role(i)
            packed += c["read_cycles"] + c["atomic_cycles"]
            new += y["read_cycles"] + y["atomic_cycles"]
            plain += y["plain_read_cycles"] + y["plain_atomic_cycles"]
        return packed, new, plain


NAMES = ["L40", "L200", "aln"]
_cache = {}


@pytest.fixture
def case(request):
    name = request.param
    if name not in _cache:
        _cache[name] = _Case(name)
    return _cache[name]


@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_renumbered_pack_oracle(gpu_ctx, case):
    got, ds, _ = case.pairs(gpu_ctx)
    ran = set(gpu_ctx.last_classes()["stem_maxk"])
    packed, new, plain = case.numbering(ds)
    err = case.oracle_err(got)
    print(f"{case.name}: classes {sorted(ran)}, model cycles plain {plain} packed {packed}, max rel err {err:.3g}")
    assert packed == new < plain  # the dataset holds the renumbered y's
    if case.name == "L200":
        assert {16, 17, 20} <= ran, ran
    assert err < 1e-6


@pytest.mark.explib
@pytest.mark.parametrize("per_item", [False, True], ids=["shared_tables", "per_item_tables"])
@pytest.mark.parametrize("case", NAMES, indirect=True)
def test_renumbered_pack_equals_plain_order(gpu_ctx, case, per_item):
    on, ds_on, sh_on = case.pairs(gpu_ctx, per_item=per_item)
    off, ds_off, sh_off = case.pairs(gpu_ctx, plain=True, per_item=per_item)
    packed_on, new, plain = case.numbering(ds_on)
    packed_off, _, _ = case.numbering(ds_off)
    assert packed_on == new < plain and packed_off == plain  # the switch selects the plain order
    if per_item:
        assert sh_on == 0 and sh_off == 0
    elif case.name != "aln":
        assert sh_on > 0 and sh_off > 0
    e_on, e_off, err = case.oracle_err(on), case.oracle_err(off), rel_err(on, off)
    print(f"{case.name}, {'per-item' if per_item else 'shared'} tables: oracle {e_on:.3g} / {e_off:.3g}, "
          f"renumbered against plain order {err:.3g}")
    assert e_on < 1e-6 and e_off < 1e-6
    assert err < 1e-12


def test_log_composition_rides_along(gpu_ctx):
    """LSuStemStrKernel (the benchmark's kernel) on the renumbered L = 40 set: both DPs reach the value."""
    items = ska.random_sequences(24, 40, SEED + 40)[:8]
    kern = ska.LSuStemStrKernel()
    ds, om = make_examples(items)
    # every ordered pair (the length band makes K(x, y) != K(y, x); a Gram would mirror its upper triangle)
    x, y = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(8), np.arange(8), indexing="ij"))
    got = gpu_ctx.pairs(ds, kern, x, y).reshape(8, 8)
    assert any(not np.array_equal(ds.y_role(i)["node"], ds.y_role(i, plain=True)["node"]) for i in range(len(items)))
    ref = np.array([[po.kernel_value(kern.params.kind, om[i], om[j], kern.params) for j in range(8)] for i in range(8)])
    err = rel_err(got, ref)
    print(f"LSuStemStrKernel: max rel err {err:.3g}")
    assert err < 1e-6
