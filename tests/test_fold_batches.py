"""The batch driver the three GPU folds share (host/fold_gpu.cpp fold_batches; host
pieces in csrc/host/fold_host.cpp): a call whose items do not fit the memory
budget together is split into batches, and the packed outputs, ln Z, the
sampled structures and the sampler's generator key (the sequence's index in
the whole call) carry on across them.  On the CPU the batch plan and the
--noLonelyPairs tables are checked on the host code alone
(tests/cpp/fold_batch_plan.cpp); on the GPU a split call must equal the
unsplit one bit for bit (experiments build: SK_FOLD_BUDGET)."""
import os
import subprocess

import numpy as np
import pytest

import stem_kernel_amd as ska

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stem_kernel_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LENGTHS = (12, 30, 30, 45, 5, 30)
BUDGET = 50000


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    """The stand-alone program over the host code: fold_host.cpp compiled
    host only (no GPU code) with the library's defines and include path."""
    exe = str(tmp_path_factory.mktemp("fold_batch_plan") / "fold_batch_plan")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "fold_batch_plan.cpp"),
                    os.path.join(CSRC, "host", "fold_host.cpp"), "-o", exe], check=True)
    return exe


def test_batch_plan(plan_exe):
    """6 n^2 + 2 (n + 1) doubles per sequence: 12 -> 7,120 bytes, 30 ->
    43,696, 45 -> 97,936, 5 -> 1,296.  Under 50,000 bytes: 12 and 30 do not
    fit together, nor 30 and 30; 45 alone is larger than the budget and still
    makes a batch (at least one item); 5 and 30 fit (44,992)."""
    out = subprocess.run([plan_exe, "plan", str(BUDGET)] + [str(n) for n in LENGTHS], check=True,
                         capture_output=True, text=True).stdout
    print(out)
    batches = [[tuple(int(v) for v in it.split(":")) for it in line.split()] for line in out.splitlines()]
    assert [[n for n, _ in b] for b in batches] == [[12], [30], [30], [45], [5, 30]]
    for b in batches:
        for n, nbytes in b:
            assert nbytes == 8 * (6 * n * n + 2 * (n + 1))
    assert batches[3][0][1] > BUDGET
    assert sum(nbytes for _, nbytes in batches[4]) <= BUDGET


def test_lonely_pair_table_of_one_row_is_the_alignment_table(plan_exe):
    """A 40-nt sequence: the fold's --noLonelyPairs table equals the consensus
    fold's of that sequence as one row and as three equal rows, with and
    without --noGU, and pairs survive in each."""
    seq = ska.random_sequences(1, 40, 0x5EED0071)[0]
    out = subprocess.run([plan_exe, "lonely", seq], check=True, capture_output=True, text=True).stdout
    print(out)
    lines = out.splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["no_gu 0", "no_gu 1"]
    pairs = [int(ln.split(":")[1].split()[0]) for ln in lines]
    assert pairs[0] >= pairs[1] > 0


def _alignment(n, rows, seed):
    """`rows` gap-free rows: a random sequence and copies with a tenth of the
    columns changed."""
    rng = np.random.default_rng(seed)
    s = ska.random_sequences(1, n, 0x5EED0080 + seed)[0]
    out = [s]
    for _ in range(rows - 1):
        r = list(s)
        for k in rng.choice(n, max(n // 10, 1), replace=False):
            r[k] = "ACGU"[int(rng.integers(0, 4))]
        out.append("".join(r))
    return out


@pytest.mark.gpu
@pytest.mark.explib
def test_gpu_split_call_equals_unsplit_call(gpu_ctx, monkeypatch, capfd):
    """Every length is at most 248, so every batch takes the ring path whatever
    its longest item is, and the tables' entries do not depend on the batch:
    bit equality.

    Plain fold, lengths (12, 30, 30, 45, 5, 30), 8 (6 n^2 + 2 (n + 1)) bytes
    each = 7,120 / 43,696 / 43,696 / 97,936 / 1,296 / 43,696: a budget of
    50,000 bytes gives the batches [12] [30] [30] [45] [5, 30].

    Sampling, 64 samples with structures: the item also counts its 64 n
    structure chars, 7,888 / 45,616 / 45,616 / 100,816 / 1,616 / 45,616: the
    same budget gives the same five batches (5 and 30: 47,232), so sequences
    1 .. 5 are keyed by their index in the call, not in their batch, and the
    structures of batch b start where those of batch b - 1 ended.

    Consensus fold, (columns, rows) = (30, 3) (12, 7) (45, 1) (30, 5), 8 (10
    n^2 + 2 (n + 1)) + n rows bytes each = 72,586 / 11,812 / 162,781 / 72,646:
    a budget of 90,000 bytes gives [(30, 3), (12, 7)] [(45, 1)] [(30, 5)].

    That the calls were split as said is read from the SK_HOST_STATS line of
    each call; that the key matters, from a call without the first sequence,
    whose samples differ."""
    seqs = [ska.random_sequences(1, n, 0x5EED0060 + k)[0] for k, n in enumerate(LENGTHS)]
    alns = [_alignment(n, rows, k) for k, (n, rows) in enumerate([(30, 3), (12, 7), (45, 1), (30, 5)])]

    def calls():
        return (gpu_ctx.fold(seqs, log_z=True),
                gpu_ctx.fold_sample(seqs, 64, seed=11, structures=True, log_z=True),
                gpu_ctx.fold_alignment(alns, with_log_z=True))

    def batches():
        return [ln.split("fold: ")[1] for ln in capfd.readouterr().err.splitlines() if "[sk] fold: " in ln]

    monkeypatch.setenv("SK_HOST_STATS", "1")
    capfd.readouterr()
    whole = calls()
    assert batches() == ["6 items in 1 batches", "6 items in 1 batches", "4 items in 1 batches"]
    monkeypatch.setenv("SK_FOLD_BUDGET", str(BUDGET))
    fold_s, sample_s, _ = calls()
    monkeypatch.setenv("SK_FOLD_BUDGET", "90000")
    ali_s = gpu_ctx.fold_alignment(alns, with_log_z=True)
    monkeypatch.delenv("SK_FOLD_BUDGET")
    # (the consensus call made under 50,000 bytes: no two alignments fit together)
    assert batches() == ["6 items in 5 batches", "6 items in 5 batches", "4 items in 4 batches",
                         "4 items in 3 batches"]
    shifted = gpu_ctx.fold_sample(seqs[1:], 64, seed=11, structures=True)[1]
    assert shifted[0] != whole[1][1][1]
    (fold_w, sample_w, ali_w) = whole

    for a, b in zip(fold_w[0], fold_s[0]):
        assert np.array_equal(a, b)
    assert np.array_equal(fold_w[1], fold_s[1])
    assert all(np.max(p) > 0 for p, n in zip(fold_w[0], LENGTHS) if n >= 30)

    bpp_w, str_w, lz_w = sample_w
    bpp_s, str_s, lz_s = sample_s
    assert str_w == str_s
    assert all(len(s) == 64 and all(len(x) == n for x in s) for s, n in zip(str_s, LENGTHS))
    for a, b in zip(bpp_w, bpp_s):
        assert np.array_equal(a, b)
    assert np.array_equal(lz_w, lz_s)
    assert any("(" in x for x in str_s[-1])

    for a, b in zip(ali_w[0], ali_s[0]):
        assert np.array_equal(a, b)
    assert np.array_equal(ali_w[1], ali_s[1])
