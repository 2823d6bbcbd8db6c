"""lbt_batch_resized_crop and ResizedCropDataset on the GPU against the numpy restatement
(tests/resized_crop_oracle.py); every output comparison is np.array_equal. The cases are those of
tests/resized_crop_cases.py (tests/test_resized_crop.py shows they reach every path of the box computation)."""
import numpy as np
import pytest
import torch

import resized_crop_cases as K
import resized_crop_oracle as R
from lbt_amd.data import ResizedCropDataset

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dataset(shape, opts, size, n=K.N_DATA, seed=1):
    X, y = K.u8(shape, n=n, seed=seed)
    C = shape[2]
    return X, y, ResizedCropDataset(X, y, K.MEAN[C], K.STD[C], size, device=DEV, **opts)


def _buffers(B, shape, offset=False):
    """(X, y) output buffers; offset: X starts 4 bytes past a 16-byte boundary."""
    n = B * int(np.prod(shape))
    buf = torch.full((n + 4,), float("nan"), dtype=torch.float32, device=DEV)
    X = buf[1:1 + n] if offset else buf[:n]
    assert X.data_ptr() % 16 == (4 if offset else 0)
    return X.view((B,) + tuple(shape)), torch.full((B,), -7, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("shape,opts", K.STORES, ids=K.STORE_IDS)
def test_resized_crop_matches_oracle(shape, opts):
    idx = torch.tensor(K.IDX, dtype=torch.int32, device=DEV)
    for size in K.OUTPUTS:
        X, y, ds = _dataset(shape, opts, size)
        k = R.of_dataset(ds)
        for augment in (True, False):
            for base in K.BASES:
                want, labels, _ = R.batch(X, y, K.IDX, size, k, augment=augment, center=ds.center, base=base,
                                          seed=K.SEED, counter=K.COUNTER)
                assert np.array_equal(labels, y[K.IDX])
                for offset in (False, True):
                    oX, oy = _buffers(len(K.IDX), ds.sample_shape, offset)
                    ds.batch(oX, oy, idx=idx, augment=augment, base=base, seed=K.SEED, counter=K.COUNTER)
                    assert np.array_equal(oX.cpu().numpy(), want), (size, augment, base, offset)
                    assert np.array_equal(oy.cpu().numpy(), labels)


def test_normalisation_and_weights_are_exact_on_every_pixel_value():
    """A store whose first image holds all 256 values per channel, resampled off the pixel grid: the
    fixture on which fp32 normalisation and truncated weights differ from the definition."""
    X, y = K.u8((16, 16, 3), n=4, seed=5)
    rng = np.random.default_rng(2)
    X[0] = np.stack([rng.permutation(256) for _ in range(3)], axis=1).reshape(16, 16, 3)
    ds = ResizedCropDataset(X, y, K.MEAN[3], K.STD[3], (11, 13), center=(13, 11), device=DEV)
    oX, oy = _buffers(4, ds.sample_shape)
    ds.batch(oX, oy)
    want, labels, _ = R.batch(X, y, range(4), (11, 13), R.of_dataset(ds), center=(13, 11))
    assert np.array_equal(oX.cpu().numpy(), want) and np.array_equal(oy.cpu().numpy(), labels)
    ident = ResizedCropDataset(X, y, K.MEAN[3], K.STD[3], 16, center=(16, 16), device=DEV)
    oX, oy = _buffers(4, (16, 16, 3))
    ident.batch(oX, oy)
    assert np.array_equal(oX.cpu().numpy(), ((X.astype(np.float64) * 65536 - ident.shift) * ident.scale_c).astype(np.float32))


def test_rows_split_into_strips_equal_the_oracle():
    """Few samples of many rows: the launch cuts every sample into strips of rows (one row each here)."""
    X, y, ds = _dataset((40, 36, 3), {}, (48, 20), n=6, seed=8)
    idx = torch.tensor([5, 0, 3], dtype=torch.int32, device=DEV)
    for augment in (True, False):
        oX, oy = _buffers(3, ds.sample_shape)
        ds.batch(oX, oy, idx=idx, augment=augment, seed=K.SEED, counter=K.COUNTER)
        want, labels, _ = R.batch(X, y, [5, 0, 3], (48, 20), R.of_dataset(ds), augment=augment, center=ds.center,
                                  seed=K.SEED, counter=K.COUNTER)
        assert np.array_equal(oX.cpu().numpy(), want) and np.array_equal(oy.cpu().numpy(), labels)


@pytest.mark.parametrize("offset", [False, True], ids=["16-byte", "4-byte"])
def test_rows_of_more_stores_than_a_workgroup_has_threads(offset):
    """Wo*C = 1044: 261 16-byte stores or 1044 4-byte stores per row against 256 threads (several passes
    over the row, the last one partial)."""
    X, y, ds = _dataset((5, 300, 3), {}, (3, 348), n=4, seed=10)
    for augment in (True, False):
        oX, oy = _buffers(2, ds.sample_shape, offset)
        ds.batch(oX, oy, first=2, augment=augment, seed=K.SEED, counter=K.COUNTER)
        want, labels, _ = R.batch(X, y, [2, 3], (3, 348), R.of_dataset(ds), augment=augment, center=ds.center,
                                  seed=K.SEED, counter=K.COUNTER)
        assert np.array_equal(oX.cpu().numpy(), want) and np.array_equal(oy.cpu().numpy(), labels)


@pytest.mark.parametrize("B", [300, 1100])  # strips of 3, 3, 3 and 1 rows; one strip of all 10 rows
def test_many_samples_take_strips_of_several_rows(B):
    X, y, ds = _dataset((6, 7, 1), {}, (10, 4), n=9, seed=9)
    src = np.random.default_rng(B).integers(0, 9, size=B)
    oX, oy = _buffers(B, ds.sample_shape)
    ds.batch(oX, oy, idx=torch.from_numpy(src.astype(np.int32)).to(DEV), augment=True, seed=K.SEED, counter=K.COUNTER)
    want, labels, _ = R.batch(X, y, src, (10, 4), R.of_dataset(ds), augment=True, seed=K.SEED, counter=K.COUNTER)
    assert np.array_equal(oX.cpu().numpy(), want) and np.array_equal(oy.cpu().numpy(), labels)


def test_two_shards_equal_one_batch():
    X, y, ds = _dataset((12, 12, 3), {}, (8, 8))
    idx = torch.tensor([3, 36, 0, 11, 11, 20, 5, 1], dtype=torch.int32, device=DEV)
    oX, oy = _buffers(8, (8, 8, 3))
    ds.batch(oX, oy, idx=idx, augment=True, seed=K.SEED, counter=K.COUNTER)
    want, labels, _ = R.batch(X, y, idx.tolist(), (8, 8), R.of_dataset(ds), augment=True, seed=K.SEED, counter=K.COUNTER)
    assert np.array_equal(oX.cpu().numpy(), want) and np.array_equal(oy.cpu().numpy(), labels)
    for r in (0, 1):
        sX, sy = _buffers(4, (8, 8, 3))
        ds.batch(sX, sy, idx=idx[4 * r:4 * r + 4], augment=True, base=4 * r, seed=K.SEED, counter=K.COUNTER)
        assert torch.equal(sX, oX[4 * r:4 * r + 4]) and torch.equal(sy, oy[4 * r:4 * r + 4])


@pytest.mark.parametrize("first", [0, 32])  # 32 + 5 == n_data
def test_resized_crop_without_index(first):
    X, y, ds = _dataset((9, 14, 3), {}, (7, 5))
    oX, oy = _buffers(5, (7, 5, 3))
    ds.batch(oX, oy, first=first, augment=True, seed=K.SEED, counter=K.COUNTER)
    want, labels, _ = R.batch(X, y, range(first, first + 5), (7, 5), R.of_dataset(ds), augment=True, seed=K.SEED,
                              counter=K.COUNTER)
    assert np.array_equal(oX.cpu().numpy(), want) and np.array_equal(oy.cpu().numpy(), labels)
    with pytest.raises(IndexError):
        ds.batch(oX, oy, first=33)
    with pytest.raises(IndexError):
        ds.batch(oX, oy, first=-1)
    with pytest.raises(IndexError):  # a caller's idx is range-checked
        ds.batch(oX, oy, idx=torch.tensor([0, 1, 2, 3, 37], dtype=torch.int32, device=DEV))


def test_out_of_range_index_gives_zeros_and_minus_one():
    X, y, ds = _dataset((12, 12, 3), {}, (8, 8))
    src = [4, 37, -1, 36, 1 << 20]
    idx = torch.tensor(src, dtype=torch.int32, device=DEV)
    for augment in (True, False):
        oX, oy = _buffers(5, (8, 8, 3))
        ds.batch(oX, oy, idx=idx, augment=augment, seed=K.SEED, counter=K.COUNTER, check=False)
        want, labels, _ = R.batch(X, y, src, (8, 8), R.of_dataset(ds), augment=augment, center=ds.center, seed=K.SEED,
                                  counter=K.COUNTER)
        assert list(labels) == [y[4], -1, -1, y[36], -1] and not want[1].any() and want[0].any()
        assert np.array_equal(oX.cpu().numpy(), want) and np.array_equal(oy.cpu().numpy(), labels)


# ------------------------------------------------------------------------------------ the Trainer
def _trainer(seed, B):
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    ctx = DfxpContext(seed=seed)
    gm = CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx)
    return ctx, Trainer(FusedResNet(gm), lr=1e-2, momentum=0.9, batch_size=B, use_graph=True)


def _bn_state(tr):
    return [t.cpu().numpy() for bn in tr._bn_layers() for t in (bn.X_mean_running, bn.X_var_running)]


def test_train_epoch_from_resized_crop_dataset_equals_hand_loop():
    """One epoch of train() (48 images stored 40x40, 32x32 batches of 16) and its evaluate() against a hand
    loop that builds every batch with the oracle and calls step(): the same parameters, momentum, exponents,
    counters and BN statistics bit for bit, and the same test accuracy."""
    m, s = K.MEAN[3], K.STD[3]
    X, y = K.u8((40, 40, 3), n=48, seed=61)
    Xte, yte = K.u8((40, 40, 3), n=24, seed=62)
    ds = ResizedCropDataset(X, y, m, s, 32, device=DEV)
    ds_te = ResizedCropDataset(Xte, yte, m, s, 32, device=DEV)
    k = R.of_dataset(ds)
    ca, ta = _trainer(61, 16)
    cb, tb = _trainer(61, 16)
    tb.dataset = (ds, ds_te)
    tb.n_epoch = 1
    torch.manual_seed(7)
    hist = tb.train(augment=True)
    torch.manual_seed(7)
    ta.get_train_op()
    perm = torch.randperm(48).numpy()
    for b in range(0, 48, 16):
        xb, yb, _ = R.batch(X, y, perm[b:b + 16], (32, 32), k, augment=True, seed=ca.seed, counter=ta.global_step)
        ta.step(torch.from_numpy(xb).to(DEV), torch.from_numpy(yb).to(DEV))
    xte, lte, _ = R.batch(Xte, yte, range(24), (32, 32), k, center=ds_te.center)
    acc, _ = ta.evaluate(xte, lte)
    torch.cuda.synchronize()
    assert hist == [acc] and ta.global_step == tb.global_step == 3 and tb.batch_sizes == [16, 16, 16]
    assert torch.equal(ta.flat.w, tb.flat.w) and torch.equal(ta.flat.a, tb.flat.a)
    assert ca.ranges() == cb.ranges() and torch.equal(ca.counts, cb.counts) and torch.equal(ca.step, cb.step)
    assert torch.equal(ca.nelem, cb.nelem)
    for u, v in zip(_bn_state(ta), _bn_state(tb)):
        assert np.array_equal(u, v)
    assert tb.evaluate(ds_te, testing=True) == ta.evaluate(xte, lte, testing=True)
