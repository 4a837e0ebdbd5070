"""The y-role numbering of the DAG stem kernel (host/pack_y.cpp pack_y,
host/pack_sweep.cpp renumber_equal_lengths): nodes are numbered by length, and the
order inside a run of equal lengths -- which fixes only a node's LDS bank, id
mod 32 as a child read and id mod 16 as an atomic target -- is chosen to lower
the bank model of the IY sweep's chunks (SweepBanks).  Host only, through
sk_dataset_y_role, which packs one example's y role in the packer's numbering
and in the plain stable order (what SK_NO_Y_RENUMBER=1 packs):

  - lengths are non-decreasing, every child id is below its parent's, and the
    new order permutes nodes within equal lengths only;
  - the chunks hold the same edges as in the plain order (the list schedule's
    composition is kept), every sweep edge sits in a later chunk than all
    edges into its child, and the length tables (lengths by id, first chunk
    by child length) are those of the plain order;
  - the model cost, restated here from the lane records, is what the library
    reports, is no higher than the plain order's for every example and lower
    over each set;
  - the packed arrays, plain and renumbered (sk_dataset_pack_digest hashes
    both), do not depend on the packing thread count.

Sets: 24 seeded synthetic sequences at L = 30, 80 and 200, and 8 three-row
alignments with gap columns at L = 64."""
import os

import numpy as np
import pytest

import stem_kernel_amd as ska
from tests.helpers import mutate_alignment

SEED = 0x5EED0002


def _sets():
    base = ska.random_sequences(8, 64, SEED + 64)
    return {
        "L30": ska.Dataset.synthetic(ska.random_sequences(24, 30, SEED + 30)),
        "L80": ska.Dataset.synthetic(ska.random_sequences(24, 80, SEED + 80)),
        "L200": ska.Dataset.synthetic(ska.random_sequences(24, 200, SEED)),
        "aln": ska.Dataset.synthetic_alignments([mutate_alignment(s, 3, SEED + k) for k, s in enumerate(base)]),
    }


@pytest.fixture(scope="module")
def packs():
    """name -> [(packer's numbering, plain order)] per example, packed once"""
    return {name: [(ds.y_role(i), ds.y_role(i, plain=True)) for i in range(len(ds))]
            for name, ds in _sets().items()}


NAMES = ["L30", "L80", "L200", "aln"]


def _fields(rec):
    return (rec & 0x7ff).astype(np.int64), ((rec >> 11) & 0x7ff).astype(np.int64), (rec >> 22).astype(np.int64)


def _model(chunk):
    """read and atomic cycles of one chunk's 64 lane records: per 32-lane half
    the most distinct children on one id mod 32, per 16-lane group the most
    records on one parent id mod 16"""
    c, p, _ = _fields(chunk)
    read = sum(max(len(set(c[h:h + 32][c[h:h + 32] % 32 == b])) for b in range(32)) for h in (0, 32))
    atomic = sum(int(np.bincount(p[g:g + 16] % 16, minlength=16).max()) for g in range(0, 64, 16))
    return read, atomic


@pytest.mark.parametrize("name", NAMES)
def test_order_is_a_permutation_within_equal_lengths(packs, name):
    changed = 0
    for new, plain in packs[name]:
        nl = len(new["node"])
        assert np.all(np.diff(new["len"].astype(np.int64)) >= 0)
        assert np.array_equal(new["len"], plain["len"])  # the kernel's first-id-by-length table follows it
        assert np.array_equal(new["first_chunk"], plain["first_chunk"])
        assert sorted(new["node"]) == list(range(nl)) == sorted(plain["node"])
        for v in np.unique(new["len"]):
            run = new["len"] == v
            assert sorted(new["node"][run]) == sorted(plain["node"][run])
        # plain: stable by length, so level-order ids ascend inside a run
        assert all(np.all(np.diff(plain["node"][plain["len"] == v].astype(np.int64)) > 0) for v in np.unique(plain["len"]))
        changed += not np.array_equal(new["node"], plain["node"])
    assert changed > 0


@pytest.mark.parametrize("name", NAMES)
def test_children_before_parents_and_same_edges(packs, name):
    for new, plain in packs[name]:
        nl = len(new["node"])
        sets = []
        for d in (new, plain):
            c, p, g = _fields(d["edges"])
            assert np.all(c < p) and (p.max(initial=0) < nl)
            assert np.all(np.diff(p) >= 0)  # node-major: parents ascend
            sets.append(sorted(zip(d["node"][c], d["node"][p], g)))
        assert sets[0] == sets[1]


@pytest.mark.parametrize("name", NAMES)
def test_sweep_chunks_keep_their_edges_and_their_order(packs, name):
    for new, plain in packs[name]:
        assert new["sweep"].shape == plain["sweep"].shape
        nl = len(new["node"])
        per_chunk = []
        for d in (new, plain):
            c, p, g = _fields(d["sweep"])
            real = c != p
            assert np.all(c[real] < p[real]) and c.max(initial=0) < nl and p.max(initial=0) < nl
            per_chunk.append([sorted(zip(d["node"][c[k][real[k]]], d["node"][p[k][real[k]]], g[k][real[k]]))
                              for k in range(c.shape[0])])
        assert per_chunk[0] == per_chunk[1]
        # the sweep's edges are the node-major edges
        c, p, g = _fields(new["sweep"])
        real = c != p
        ce, pe, ge = _fields(new["edges"])
        assert sorted(zip(c[real], p[real], g[real])) == sorted(zip(ce, pe, ge))
        # every edge after all edges into its child: last chunk that adds into a node < first that reads it
        chunk = np.repeat(np.arange(c.shape[0]), 64).reshape(c.shape)
        last_in = np.full(nl, -1)
        np.maximum.at(last_in, p[real], chunk[real])
        assert np.all(chunk[real] > last_in[c[real]])


@pytest.mark.parametrize("name", NAMES)
def test_model_cost_no_higher_per_example_and_lower_over_the_set(packs, name):
    tot_new = tot_plain = 0
    for new, plain in packs[name]:
        for d in (new, plain):
            cost = [_model(ch) for ch in d["sweep"]]
            assert (sum(r for r, _ in cost), sum(a for _, a in cost)) == (d["read_cycles"], d["atomic_cycles"])
            assert d["read_cycles"] >= 2 * len(cost) and d["atomic_cycles"] >= 4 * len(cost)
        assert (new["plain_read_cycles"], new["plain_atomic_cycles"]) == (plain["read_cycles"], plain["atomic_cycles"])
        a, b = new["read_cycles"] + new["atomic_cycles"], plain["read_cycles"] + plain["atomic_cycles"]
        assert a <= b
        if np.array_equal(new["node"], plain["node"]):
            assert a == b
        tot_new += a
        tot_plain += b
    print(f"{name}: model cycles {tot_plain} -> {tot_new} ({tot_new / tot_plain - 1:+.1%})")
    assert tot_new < tot_plain


def test_pack_independent_of_thread_count():
    seqs = ska.random_sequences(40, 120, SEED + 120)
    saved = os.environ.get("SK_PACK_THREADS")
    try:
        digests = []
        for t in ("1", "8"):
            os.environ["SK_PACK_THREADS"] = t
            digests.append(ska.Dataset.synthetic(seqs).pack_digest())
    finally:
        os.environ.pop("SK_PACK_THREADS", None)
        if saved is not None:
            os.environ["SK_PACK_THREADS"] = saved
    assert digests[0] == digests[1]
