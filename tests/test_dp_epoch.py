"""Data-parallel epochs, the parts that need no GPU (lbt_amd/trainer.py: shard_rows, check_epoch_shards,
decode_tally; the two new entry points' exports and host-side argument checks).

The GPU side is tests/test_dp_epoch_kernels_gpu.py (the kernels) and tests/test_dp_epoch_gpu.py (two ranks
against one process).
"""
import ctypes
import os

import numpy as np
import pytest

import eval_oracle as E
from lbt_amd import _lib
from lbt_amd.trainer import check_epoch_shards, decode_tally, epoch_batch_sizes, shard_rows

NEW = ("lbt_augment_flip_crop_at", "lbt_eval_tally")
EINVAL = 1001


# ---------------------------------------------------------------- shard arithmetic
@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_shard_rows_grid(world):
    """Rank r takes rows [r * nb / world, (r + 1) * nb / world): for every divisible nb of a small grid the
    shards are equal, disjoint, in rank order, and cover the batch."""
    for nb in range(0, 5 * world + 1, world):
        seen = []
        for rank in range(world):
            lo, hi = shard_rows(nb, world, rank)
            assert (lo, hi) == (rank * nb // world, (rank + 1) * nb // world)
            assert hi - lo == nb // world
            assert list(range(lo, hi)) == E.shard(nb, world, rank)
            seen += list(range(lo, hi))
        assert seen == list(range(nb)), (nb, world)


def test_shard_rows_refuses_uneven_batches_and_bad_ranks():
    for nb, world in ((1, 2), (3, 2), (16, 3), (7, 8), (9, 4)):
        for rank in range(world):
            with pytest.raises(ValueError, match="equal shards"):
                shard_rows(nb, world, rank)
    for world, rank in ((2, 2), (2, -1), (0, 0), (1, 1)):
        with pytest.raises(ValueError, match="world"):
            shard_rows(8, world, rank)


def test_epoch_batch_sizes_and_the_up_front_check():
    assert epoch_batch_sizes(80, 32) == [32, 16]
    assert epoch_batch_sizes(64, 32) == [32]
    assert epoch_batch_sizes(10, 32) == [10]
    assert epoch_batch_sizes(48, 16) == [16]
    with pytest.raises(ValueError):
        epoch_batch_sizes(10, 0)
    for n, bs, world in ((80, 32, 2), (80, 32, 4), (80, 32, 16), (64, 32, 32), (5, 7, 1), (48, 16, 8)):
        check_epoch_shards(n, bs, world)  # every size divisible: silent
    for n, bs, world in ((80, 32, 32), (81, 32, 2), (80, 30, 4), (10, 32, 4), (80, 33, 2)):
        with pytest.raises(ValueError) as e:
            check_epoch_shards(n, bs, world)
        msg = str(e.value)
        assert "n = %d" % n in msg and "batch_size = %d" % bs in msg and "world = %d" % world in msg


class _Untouchable:
    """A dataset array that knows its length and fails on any other use."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        raise AssertionError("the dataset was touched before the up-front check")

    def __array__(self, *a, **k):
        raise AssertionError("the dataset was touched before the up-front check")


def test_train_checks_every_batch_size_before_the_dataset_is_touched(monkeypatch):
    """train() on a trainer that shards over 2 ranks raises the ValueError for n = 81 (final batch of 17)
    before it draws the permutation, rebuilds the optimiser or reads a sample; the same trainer without
    sharding goes on (and then does touch the dataset)."""
    import torch

    from lbt_amd.models import MNIST_Model
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    tr = Trainer(MNIST_Model(8, dropout=1.0, ctx=DfxpContext(device="cpu")), use_graph=False, batch_size=32, n_epoch=1,
                 dataset=((_Untouchable(81), _Untouchable(81)), (None, None)))
    assert tr.world == 1 and tr.rank == 0 and not tr._shard and tr._shard_of(17) == (0, 17)
    drawn = []

    def randperm(n):
        drawn.append(n)
        raise AssertionError("drawn")
    monkeypatch.setattr(torch, "randperm", randperm)
    monkeypatch.setattr(tr, "get_train_op", lambda: drawn.append("op"))
    tr.world, tr._shard = 2, True  # what a two-rank process group makes of it
    with pytest.raises(ValueError) as e:
        tr.train()
    assert "n = 81" in str(e.value) and "batch_size = 32" in str(e.value) and "world = 2" in str(e.value)
    assert drawn == []
    tr.world, tr._shard = 1, False
    with pytest.raises(AssertionError, match="drawn"):  # one process: no check, the loop starts
        tr.train()
    assert drawn == ["op", 81]


# ---------------------------------------------------------------- tally rows -> (accuracy, loss)
def test_decode_tally_against_the_numpy_restatement():
    rng = np.random.default_rng(5)
    for nbatches in (1, 2, 3, 11):
        sizes = [int(s) for s in rng.integers(1, 1001, nbatches)]
        rows = [[int(rng.integers(0, s + 1)), int(rng.integers(0, 1 << 45))] for s in sizes]
        assert decode_tally(rows, sizes) == E.decode(rows, sizes)
    # the reference's shape: 10 batches of 1000, a third of them right, a loss near ln 10
    sizes = [1000] * 10
    rows = [[333 + i, int((2.302585 + 0.01 * i) * 1000 * 2 ** 32)] for i in range(10)]
    acc, loss = decode_tally(rows, sizes)
    assert (acc, loss) == E.decode(rows, sizes)
    assert abs(acc - 0.3375) < 1e-6 and abs(loss - 2.347585) < 1e-5
    # per batch: fp32 of the exact quotient, not a double division
    assert decode_tally([[1, 0]], [3]) == (float(np.float32(1) / np.float32(3)), 0.0)
    assert decode_tally([[2, 3 << 32]], [3])[1] == 1.0
    assert decode_tally([], []) == (0.0, 0.0)
    with pytest.raises(ValueError):
        decode_tally([[1, 2]], [])


def test_sharded_rows_sum_to_the_batch_row():
    """The integers survive the sum over the ranks: per-shard correct counts add to the batch's, so the
    decoded accuracy of the summed row is the whole batch's fp32 mean of 0 / 1."""
    rng = np.random.default_rng(9)
    logits = rng.standard_normal((40, 10)).astype(np.float32)
    logits[3, 2] = logits[3, 7] = logits[3].max() + 1  # a tie: the lower index counts
    labels = rng.integers(0, 10, 40).astype(np.int32)
    labels[3] = 2
    for world in (1, 2, 4, 8):
        total = 0
        for r in range(world):
            idx = E.shard(40, world, r)
            total += E.correct(logits[idx], labels[idx])
        assert total == E.correct(logits, labels)
        want = float((np.argmax(logits, axis=1) == labels).astype(np.float32).mean(dtype=np.float32))
        assert decode_tally([[total, 0]], [40])[0] == want


# ---------------------------------------------------------------- ABI and host-side checks
def test_new_symbols_are_exported_and_declared():
    """The header declares both entry points and the bindings export them (test_abi.py holds header ==
    bindings); they are additions under the ABI number the library and the bindings agree on."""
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "lbt_dfxp.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(lib, name), name
        assert "int %s(" % name in header, name
    assert lib.lbt_abi_version() == _lib.ABI_VERSION


def test_augment_at_host_side_checks():
    """Rejected before any HIP call (no GPU here; the pointers are never dereferenced): the plain call's
    checks at a base, base < 0, base + N > 2^32."""
    lib = _lib.load()
    x, y = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)
    N = 6
    for base in (-1, -6, (1 << 32) - N + 1, 1 << 32, 1 << 40, 1 << 62):
        assert lib.lbt_augment_flip_crop_at(x, y, N, 8, 8, 3, 4, base, 1, 2, None) == EINVAL, base
    for args in ((0, 8, 8, 3, 4), (-1, 8, 8, 3, 4), (N, 0, 8, 3, 4), (N, 8, 0, 3, 4), (N, 8, 8, 0, 4), (N, 8, 8, 3, -1)):
        for base in (0, 4):
            assert lib.lbt_augment_flip_crop_at(x, y, *args, base, 1, 2, None) == EINVAL, (args, base)
    assert lib.lbt_augment_flip_crop_at(x, x, N, 8, 8, 3, 4, 4, 1, 2, None) == EINVAL  # in place
    assert lib.lbt_augment_flip_crop(x, x, N, 8, 8, 3, 4, 1, 2, None) == EINVAL  # (the plain call, unchanged)


def test_eval_tally_host_side_checks():
    lib = _lib.load()
    p = ctypes.c_void_p(0x1000)
    assert lib.lbt_eval_tally(None, p, 4, 10, p, None) == EINVAL
    assert lib.lbt_eval_tally(p, None, 4, 10, p, None) == EINVAL
    assert lib.lbt_eval_tally(p, p, 4, 10, None, None) == EINVAL
    for B in (0, -1):
        assert lib.lbt_eval_tally(p, p, B, 10, p, None) == EINVAL
    for K in (0, -3):
        assert lib.lbt_eval_tally(p, p, 4, K, p, None) == EINVAL
