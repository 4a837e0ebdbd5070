"""Every kernel a fold launch can run, against the oracle, under every flag.

The fold picks its kernel per launch from the launch's longest item
(csrc/kernels/fold.hip fold_path, fold_ali.hip fold_ali_path):

* `ring`  sk_fold_kernel<true, false> / sk_fold_ali_kernel<true>: up to 248
          nucleotides, the interior-loop window in an LDS ring of 33 diagonals;
* `hbm`   sk_fold_kernel<false, false> / sk_fold_ali_kernel<false>: no ring,
          the Boltzmann tables in LDS;
* `gtab`  sk_fold_kernel<false, true>: no ring, the hairpin and scale tables
          read from HBM.  A launch takes it by itself only when 8 n_tab_pad +
          the padded codes pass 163,584 bytes; n_tab = 151 + (L + 2) + (L + 3),
          so 8 (2 L + 156) + L > 163,584 from L = 9,550 on, far past the ~1,400
          nucleotides at which Z leaves the double range.  Only the experiments
          build's SK_FOLD_PATH reaches it.

So one long sequence in a call takes every other sequence of that call off the
ring.  Each test here reads the path that ran from the batch driver's
SK_HOST_STATS line (tests/helpers.py fold_paths) and asserts it.

References and tolerances are test_fold.py's: the oracle's DP
(oracle/fold_oracle.c) at 1e-9 absolute on probabilities and 1e-12 relative on
ln Z, its enumeration at 1e-12 / 1e-12; flags are (no_gu, no_closing_gu,
no_lonely_pairs), the five sets test_oracle_dp_equals_enumeration pins on the
CPU.  The consensus fold's ring / hbm cases are in test_alifold.py, the
sampler's after an hbm inside launch in test_fold_sample.py."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import test_alifold as tal
from tests import test_fold_sample as tfs
from tests.helpers import fold_paths

FLAGS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]
MIX = "ACGUNNacgut-ggccAAAUUUggcc"  # test_gpu_fold_matches_oracle's: unpairable and lower-case characters
# 33 / 34: the first wrap of the 33-slot ring; 36 / 37: the 30-nt interior
# window first full; 247 / 248: the longest the ring takes
RING_LENGTHS = (5, 17, 33, 34, 36, 37, 66, 130, 200, 247, 248)
FORCED_LENGTHS = (17, 36, 130, 248)
HAIRPIN12 = "GGGUGAAAUCCC"


@functools.lru_cache(maxsize=None)
def _seq(L):
    """one fixed random sequence per length"""
    return "".join(np.random.default_rng(0xF01D + L).choice(list("ACGU"), L))


@functools.lru_cache(maxsize=None)
def _oracle(seq, flags):
    """(ln Z, bpp) of the oracle's DP, computed once per (sequence, flags)"""
    lz, p = po.fold_mccaskill(seq, flags[0], flags[1], no_lp=bool(flags[2]))
    p.setflags(write=False)
    return lz, p


def _kw(f):
    return dict(no_gu=bool(f[0]), no_closing_gu=bool(f[1]), no_lonely_pairs=bool(f[2]))


def _check(seq, p, z, flags):
    ref_z, ref_p = _oracle(seq, flags)
    assert abs(z - ref_z) <= 1e-12 * max(1.0, abs(ref_z)), (len(seq), flags, z, ref_z)
    assert p.shape == ref_p.shape
    assert np.max(np.abs(p - ref_p), initial=0.0) < 1e-9, (len(seq), flags)
    if len(seq) <= 17:
        b, pb, _ = po.fold_enum(seq, flags[0], flags[1], no_lp=bool(flags[2]))
        assert abs(z - b) < 1e-12 * max(1.0, abs(b)), (seq, flags)
        assert np.max(np.abs(p - pb), initial=0.0) < 1e-12, (seq, flags)


def _fold(ctx, capfd, monkeypatch, seqs, flags):
    (p, lz), batches = fold_paths(capfd, monkeypatch, lambda: ctx.fold(seqs, log_z=True, **_kw(flags)))
    return p, lz, batches


# ------------------------------------------------------------------ shipped library
@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS)
def test_gpu_ring_path_matches_oracle(gpu_ctx, monkeypatch, capfd, flags):
    """One launch on the ring; MIX (26 characters) and every length but 248
    have rows shorter than the ring's stride, the launch's longest item."""
    seqs = [_seq(L) for L in RING_LENGTHS] + [MIX]
    got, lz, batches = _fold(gpu_ctx, capfd, monkeypatch, seqs, flags)
    assert batches == [(len(seqs), 248, "ring")]
    for s, p, z in zip(seqs, got, lz):
        _check(s, p, z, flags)
    assert max(np.max(p, initial=0.0) for p in got) > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS)
def test_gpu_ring_boundary(gpu_ctx, monkeypatch, capfd, flags):
    """248 nucleotides alone run the ring kernel, 249 the one without it, and
    a 12-mer in the call of the 249-mer leaves the ring with it: the same
    result as alone (on the ring) to 1e-13, the figure of
    test_gpu_fold_tables_sized_per_batch."""
    for L, path in ((248, "ring"), (249, "hbm")):
        got, lz, batches = _fold(gpu_ctx, capfd, monkeypatch, [_seq(L)], flags)
        assert batches == [(1, L, path)]
        _check(_seq(L), got[0], lz[0], flags)
    solo, lz_s, batches = _fold(gpu_ctx, capfd, monkeypatch, [HAIRPIN12], flags)
    assert batches == [(1, 12, "ring")]
    both, lz_b, batches = _fold(gpu_ctx, capfd, monkeypatch, [HAIRPIN12, _seq(249)], flags)
    assert batches == [(2, 249, "hbm")]
    _check(HAIRPIN12, both[0], lz_b[0], flags)
    _check(_seq(249), both[1], lz_b[1], flags)
    assert np.max(both[0]) > 0.1
    assert np.max(np.abs(solo[0] - both[0])) < 1e-13 and abs(lz_s[0] - lz_b[0]) <= 1e-13 * abs(lz_s[0])


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [(0, 0, 0), (1, 1, 1)])
def test_gpu_spans_of_more_than_one_trip(gpu_ctx, monkeypatch, capfd, flags):
    """530 nucleotides: the spans d = 4 .. 17 have 526 .. 513 cells, more than
    the block's 512 threads, so the inside and the outside pass make a second
    trip over them; the probabilities come from both passes."""
    s = _seq(530)
    got, lz, batches = _fold(gpu_ctx, capfd, monkeypatch, [s], flags)
    assert batches == [(1, 530, "hbm")]
    _check(s, got[0], lz[0], flags)
    n = len(s)
    P = np.zeros((n, n))
    P[np.triu_indices(n, 1)] = got[0]
    assert np.all(got[0] >= 0) and np.max((P + P.T).sum(1)) <= 1 + 1e-12
    assert np.max(got[0]) > 0.1


# ------------------------------------------------------------------ experiments build: forced paths
@pytest.mark.gpu
@pytest.mark.explib
@pytest.mark.parametrize("flags", FLAGS)
def test_gpu_forced_paths_match_oracle(gpu_ctx, monkeypatch, capfd, flags):
    """The same short sequences on the ring, without it (SK_FOLD_PATH=hbm) and
    with the hairpin / scale tables in HBM (gtab, which no input that stays in
    the double range selects): each against the oracle, and the three equal
    to the last bit -- where a value is kept changes no operation and no order
    of a sum (measured on the MI355X under all five flag sets: every
    difference 0), so array_equal stands for the 1e-13 a reordering would need."""
    seqs = [_seq(L) for L in FORCED_LENGTHS] + [MIX]
    runs = {}
    for path in ("ring", "hbm", "gtab"):
        if path != "ring":
            monkeypatch.setenv("SK_FOLD_PATH", path)
        got, lz, batches = _fold(gpu_ctx, capfd, monkeypatch, seqs, flags)
        monkeypatch.delenv("SK_FOLD_PATH", raising=False)
        assert batches == [(len(seqs), 248, path)]
        for s, p, z in zip(seqs, got, lz):
            _check(s, p, z, flags)
        runs[path] = (got, lz)
    for other in ("hbm", "gtab"):
        for k in range(len(seqs)):
            diff = float(np.max(np.abs(runs["ring"][0][k] - runs[other][0][k])))
            assert np.array_equal(runs["ring"][0][k], runs[other][0][k]), (other, len(seqs[k]), diff)
        assert np.array_equal(runs["ring"][1], runs[other][1]), (other, runs["ring"][1] - runs[other][1])


@pytest.mark.gpu
@pytest.mark.explib
def test_gpu_unknown_forced_path_is_an_error(gpu_ctx, monkeypatch):
    import stem_kernel_amd as ska
    monkeypatch.setenv("SK_FOLD_PATH", "ring")  # the ring cannot be asked for
    with pytest.raises(ska.StemKernelError) as e:
        gpu_ctx.fold([HAIRPIN12])
    assert e.value.code == -1 and "SK_FOLD_PATH" in str(e.value)


@pytest.mark.gpu
@pytest.mark.explib
@pytest.mark.parametrize("f", tfs.FLAGS)
def test_gpu_pair_marginals_after_gtab_inside_launch(gpu_ctx, monkeypatch, capfd, f):
    """The sampler walks the inside tables a gtab launch left (its own tables
    stay in LDS): test_fold_sample.py's binomial bound and sequence."""
    seq, s = tfs._random(75), 8192
    monkeypatch.setenv("SK_FOLD_PATH", "gtab")
    (bpp, lz), batches = fold_paths(capfd, monkeypatch,
                                    lambda: gpu_ctx.fold_sample([seq], s, seed=3, log_z=True, **tfs._kw(f)))
    monkeypatch.delenv("SK_FOLD_PATH")
    assert batches == [(1, 75, "gtab")]
    ref_z, ref = tfs._oracle(seq, f)
    dev, lim = np.abs(bpp[0] - ref), tfs._bound(ref, s)
    print(f"L=75 {f}: worst deviation {np.max(dev / lim):.3f} of the bound")
    assert np.all(dev <= lim) and np.count_nonzero(bpp[0]) > 0
    assert abs(lz[0] - ref_z) <= 1e-12 * abs(ref_z)


@pytest.mark.gpu
@pytest.mark.explib
@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True)])
def test_gpu_consensus_fold_off_the_ring(gpu_ctx, monkeypatch, capfd, flags):
    """sk_fold_ali_kernel<false> on short alignments (SK_FOLD_PATH=hbm):
    test_alifold.py's named alignments against the enumeration and its 70
    columns x 7 rows against the DP; gtab is not the consensus fold's to take."""
    names = list(tal.ALNS)
    rows70 = tal._mutated_alignment(np.random.default_rng(970), 70, 7)
    alns = [tal.ALNS[k] for k in names] + [rows70]
    kw = dict(no_gu=flags[0], no_lonely_pairs=flags[1], with_log_z=True)
    monkeypatch.setenv("SK_FOLD_PATH", "hbm")
    (got, lz), batches = fold_paths(capfd, monkeypatch, lambda: gpu_ctx.fold_alignment(alns, **kw))
    monkeypatch.setenv("SK_FOLD_PATH", "gtab")
    (got_g, lz_g), batches_g = fold_paths(capfd, monkeypatch, lambda: gpu_ctx.fold_alignment(alns, **kw))
    monkeypatch.delenv("SK_FOLD_PATH")
    assert batches == [(len(alns), 70, "hbm")] and batches_g == [(len(alns), 70, "ring")]
    for k, name in enumerate(names):
        ref_z, ref_p, _, _ = tal._enum(tuple(tal.ALNS[name]), *flags)
        tal._close(lz[k], got[k], ref_z, ref_p)
        tal._close(lz_g[k], got_g[k], ref_z, ref_p)
    ref_z, ref_p = tal._dp(tuple(rows70), *flags)
    assert np.max(ref_p) > 0.1
    tal._close(lz[-1], got[-1], ref_z, ref_p)
    tal._close(lz_g[-1], got_g[-1], ref_z, ref_p)
