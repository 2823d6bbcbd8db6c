"""The two kernels of the data-parallel epoch on the GPU, one process (lbt_amd/csrc/aux.hip, eval.hip).

* lbt_augment_flip_crop_at: rows [base, base + B) of the plain call on a whole batch equal the call on those
  rows at that base bit for bit; base 0 is the plain entry point; the numpy oracle's draws.
* lbt_eval_tally: the first-maximum count against numpy on crafted ties, the fixed-point loss sum against
  lbt_softmax_xent_n's loss_fx on the same inputs exactly (both of its paths), nothing written around row.
"""
import ctypes

import numpy as np
import pytest
import torch

import eval_oracle as E
from lbt_amd import _lib
from oracle import aux as oaux

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, COUNTER = 1234, 77


# ---------------------------------------------------------------- lbt_augment_flip_crop_at
def _images(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


@pytest.mark.parametrize("shape,pad", [((6, 8, 8, 3), 4), ((6, 5, 7, 1), 2)])
def test_augment_at_equals_the_rows_of_the_whole_batch(shape, pad):
    from lbt_amd.dfxp import ops
    x = _images(shape, 3)
    xd = torch.from_numpy(x).to(DEV)
    full = ops.augment_flip_crop(xd, pad, SEED, COUNTER).cpu().numpy()
    assert np.array_equal(full, oaux.augment_flip_crop(x, pad, SEED, COUNTER))
    assert not np.array_equal(full, x)  # the draws move something
    for base in (0, 1, 4):
        for B in sorted({1, 2, shape[0] - base}):
            rows = xd[base:base + B].contiguous()
            got = ops.augment_flip_crop(rows, pad, SEED, COUNTER, base=base).cpu().numpy()
            assert np.array_equal(got, full[base:base + B]), (base, B)
            # the entry point itself, base 0 included (ops takes the plain entry point there)
            out = torch.full_like(rows, 7.0)
            _lib.call("lbt_augment_flip_crop_at", _lib.ptr(rows), _lib.ptr(out), B, shape[1], shape[2], shape[3], pad,
                      base, SEED, COUNTER, _lib.stream())
            assert np.array_equal(out.cpu().numpy(), full[base:base + B]), (base, B)
    # a shard's own draws differ from the draws it would make as a batch of its own
    own = ops.augment_flip_crop(xd[4:6].contiguous(), pad, SEED, COUNTER).cpu().numpy()
    assert not np.array_equal(own, full[4:6])


def test_augment_at_rejects_bad_arguments_before_launching():
    x = torch.zeros((6, 8, 8, 3), device=DEV)
    y = torch.full_like(x, 3.0)
    lib = _lib.load()
    st = _lib.stream()
    for base in (-1, (1 << 32) - 5, 1 << 33):
        assert lib.lbt_augment_flip_crop_at(_lib.ptr(x), _lib.ptr(y), 6, 8, 8, 3, 4, base, 1, 2, st) == 1001
    assert lib.lbt_augment_flip_crop_at(_lib.ptr(x), _lib.ptr(x), 6, 8, 8, 3, 4, 0, 1, 2, st) == 1001
    assert lib.lbt_augment_flip_crop_at(_lib.ptr(x), _lib.ptr(y), 6, 8, 8, 3, -1, 0, 1, 2, st) == 1001
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())  # nothing ran
    # the last accepted base
    assert lib.lbt_augment_flip_crop_at(_lib.ptr(x), _lib.ptr(y), 6, 8, 8, 3, 4, (1 << 32) - 6, 1, 2, st) == 0
    torch.cuda.synchronize()
    assert bool((y == 0.0).all())


# ---------------------------------------------------------------- lbt_eval_tally
def _tally_case(B, K, seed):
    """Logits with crafted ties in the first rows (as many as B allows): two and three equal maxima, the label
    at the lower and at the higher index; the rest random with random labels (about 1 / K right)."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, K)).astype(np.float32)
    y = rng.integers(0, K, B).astype(np.int32)
    hi, mid = K - 1, K // 2
    ties = [((1, hi), 1), ((1, hi), hi), ((0, mid, hi), 0), ((0, mid, hi), mid), ((0, mid, hi), hi),
            ((mid, hi), mid), ((mid, hi), hi)]
    for r, (cols, label) in enumerate(ties[:B]):
        z[r, list(cols)] = np.float32(z[r].max() + 1.5)
        y[r] = label
    if B > len(ties):  # some plainly right rows too
        for r in range(len(ties), min(B, len(ties) + 3)):
            y[r] = int(np.argmax(z[r]))
    return z, y


def _run_tally(z, y):
    """(row, loss_fx of lbt_softmax_xent_n, the poisoned words around row)."""
    B, K = z.shape
    zd, yd = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    poison = -0x0101010101010102
    buf = torch.full((6,), poison, dtype=torch.int64, device=DEV)
    row = buf[2:4]
    _lib.call("lbt_eval_tally", _lib.ptr(zd), _lib.ptr(yd), B, K, _lib.ptr(row), _lib.stream())
    loss = torch.zeros(1, device=DEV)
    dz = torch.empty_like(zd)
    fx = torch.zeros(1, dtype=torch.int64, device=DEV)
    _lib.call("lbt_softmax_xent_n", _lib.ptr(zd), _lib.ptr(yd), B, K, B, _lib.ptr(loss), _lib.ptr(dz), _lib.ptr(fx),
              _lib.stream())
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.array_equal(zd.cpu().numpy(), z) and np.array_equal(yd.cpu().numpy(), y)  # sources read only
    return out[2:4].tolist(), int(fx.item()), out[[0, 1, 4, 5]].tolist(), poison, float(loss.item())


@pytest.mark.parametrize("B,K", [(1, 10), (37, 10), (5, 1000), (300, 10), (37, 64), (21, 65), (3, 1500)])
def test_eval_tally_counts_first_maxima_and_restates_the_loss_sum(B, K):
    """The issue's three shapes, and the sizes at which the code takes another path: more rows than threads
    (300), both sides of the classes <= 64 split (64, 65), more rows than waves on the wide path (21), and a
    head wider than the softmax kernel's register path (1500 > 1024)."""
    z, y = _tally_case(B, K, 100 * B + K)
    row, fx, around, poison, loss = _run_tally(z, y)
    want = E.correct(z, y)
    assert 0 < want or B == 1
    assert row[0] == want
    assert row[1] == fx  # bit for bit the softmax kernel's fixed-point sum
    assert around == [poison] * 4
    # and the sum is the loss: decoded as the trainer decodes it, against float64 numpy
    zz = z.astype(np.float64)
    ref = float(np.mean(np.log(np.exp(zz - zz.max(1, keepdims=True)).sum(1)) + zz.max(1) - zz[np.arange(B), y]))
    from lbt_amd.trainer import decode_tally
    acc, got = decode_tally([row], [B])
    assert acc == float(np.float32(want) / np.float32(B))
    assert abs(got - ref) <= 1e-5 * abs(ref) + 1e-6 and abs(got - loss) <= 1e-6 * abs(loss) + 1e-9


def test_eval_tally_shards_sum_to_the_whole_batch():
    """Two ranks' rows added: the correct count is the batch's; the loss sums differ from the whole batch's
    fixed-point sum by at most the two extra roundings to 2^-32 (and the order of the double additions)."""
    z, y = _tally_case(40, 10, 8)
    whole, _, _, _, _ = _run_tally(z, y)
    a, _, _, _, _ = _run_tally(z[:20].copy(), y[:20].copy())
    b, _, _, _, _ = _run_tally(z[20:].copy(), y[20:].copy())
    assert a[0] + b[0] == whole[0] == E.correct(z, y)
    assert abs(a[1] + b[1] - whole[1]) <= 2 + whole[1] * 2.0 ** -50


def test_eval_tally_rejects_bad_arguments_before_launching():
    lib = _lib.load()
    z = torch.zeros((4, 10), device=DEV)
    y = torch.zeros(4, dtype=torch.int32, device=DEV)
    row = torch.full((2,), 5, dtype=torch.int64, device=DEV)
    st = _lib.stream()
    P = _lib.ptr
    assert lib.lbt_eval_tally(None, P(y), 4, 10, P(row), st) == 1001
    assert lib.lbt_eval_tally(P(z), None, 4, 10, P(row), st) == 1001
    assert lib.lbt_eval_tally(P(z), P(y), 4, 10, None, st) == 1001
    assert lib.lbt_eval_tally(P(z), P(y), 0, 10, P(row), st) == 1001
    assert lib.lbt_eval_tally(P(z), P(y), -4, 10, P(row), st) == 1001
    assert lib.lbt_eval_tally(P(z), P(y), 4, 0, P(row), st) == 1001
    torch.cuda.synchronize()
    assert row.tolist() == [5, 5]
    # ops.eval_tally: the typed wrapper; all-equal logits -> every row's first maximum is class 0
    from lbt_amd.dfxp import ops
    ops.eval_tally(z, y, row)
    torch.cuda.synchronize()
    assert row.tolist()[0] == 4 and abs(row.tolist()[1] * 2.0 ** -32 / 4 - np.log(10)) < 1e-6
    with pytest.raises(ValueError):
        ops.eval_tally(z, y, torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ops.eval_tally(z, y.to(torch.int64), row)
