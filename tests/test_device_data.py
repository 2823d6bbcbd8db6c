"""Device-resident datasets (lbt_amd/data.py, lbt_batch_gather, Trainer.train / evaluate on a DeviceDataset).

The yardstick is the host path: load_data's float64 normalisation (main.py:65-75), a numpy gather, and
preprocess_image as oracle.aux.augment_flip_crop restates it (trainer.py:24-28). Every comparison is
np.array_equal."""
import ctypes

import numpy as np
import pytest
import torch

from lbt_amd import _lib
from lbt_amd.data import DeviceDataset
from oracle import aux as oaux

F32 = np.float32
DEV = "cuda:0"
N_DATA = 37
IDX = [36, 0, 7, 7, 19]  # a repeat, both ends, unordered
SEED = 0x0123456789ABCDEF  # both key words in use
COUNTER = (1 << 32) + 77  # both counter words in use
SHAPES = [(8, 8, 3), (5, 7, 3), (6, 6, 1), (4, 4, 4), (1, 1, 20)]  # (8,8,3): 16-byte rows; (5,7,3): W*C = 21


def _u8(shape, n=N_DATA, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, size=(n,) + tuple(shape), dtype=np.uint8),
            rng.integers(0, 10, size=n).astype(np.int32))


def _norm(X, mean):
    """load_data: float64 subtract and divide, one rounding to fp32 at the feed."""
    return ((X.astype(np.float64) - mean) / 128).astype(F32)


def _norm_fixture():
    """uint8 images [37, 8, 8, 4] whose first image holds all 256 values, with their own mean (sums over
    37: non-terminating binary fractions)."""
    X, y = _u8((8, 8, 4), seed=6)
    X[0] = np.arange(256, dtype=np.uint8).reshape(8, 8, 4)
    return X, y, X.mean(axis=0, dtype=np.float64)


def _oracle(xn, pad, flip, base, seed=SEED, counter=COUNTER):
    """preprocess_image of the normalised batch xn with the draws of samples base .. base + B - 1; flip off:
    the drawn flips are undone beforehand (a flip is its own inverse), which leaves the crop alone."""
    B = len(xn)
    full = np.zeros((base + B,) + xn.shape[1:], dtype=F32)  # `base` dummy leading rows
    full[base:] = xn
    if not flip:
        drawn, _, _ = oaux.augment_draws(base + B, pad, seed, counter)
        for n in range(base, base + B):
            if drawn[n]:
                full[n] = full[n][:, ::-1]
    return oaux.augment_flip_crop(full, pad, seed, counter)[base:]


# ------------------------------------------------------------------------------------ CPU
def _gather_args(**over):
    """A full argument list of lbt_batch_gather with fake non-NULL pointers (never dereferenced: every
    case below is rejected on the host first)."""
    p = ctypes.c_void_p(0x1000)
    a = dict(data=p, src_kind=0, mean=p, labels=p, n_data=37, idx=None, first=0, X=p, y=p, B=5, H=8, W=8, C=3,
             pad=4, flip=1, base=0, seed=1, counter=2)
    a.update(over)
    return [a[k] for k in ("data", "src_kind", "mean", "labels", "n_data", "idx", "first", "X", "y", "B", "H", "W", "C",
                           "pad", "flip", "base", "seed", "counter")] + [None]


EINVAL_CASES = [dict(data=None), dict(labels=None), dict(X=None), dict(y=None), dict(mean=None), dict(src_kind=2),
                dict(src_kind=-1), dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(C=0), dict(C=-3), dict(n_data=0),
                dict(n_data=-5), dict(pad=-1), dict(pad=32768), dict(base=-1), dict(base=(1 << 32) - 4),
                dict(base=1 << 40), dict(first=-1), dict(first=33), dict(first=1 << 40),
                dict(H=1 << 11, W=1 << 10, C=1 << 10), dict(H=1 << 16, W=1 << 16, C=1),
                dict(src_kind=1, mean=None, first=33)]


@pytest.mark.parametrize("over", EINVAL_CASES, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_batch_gather_host_checks_return_einval(over):
    assert _lib.load().lbt_batch_gather(*_gather_args(**over)) == 1001


def test_device_dataset_argument_checks():
    X, y = _u8((4, 4, 3), n=6)
    for bad in (X.astype(np.int16), X.astype(np.float64), X.astype(np.float16)):
        with pytest.raises(TypeError):
            DeviceDataset(bad, y, device="cpu")
    with pytest.raises(ValueError):
        DeviceDataset(X, y[:5], device="cpu")
    with pytest.raises(ValueError):
        DeviceDataset(X.astype(F32), y, mean=np.zeros((4, 4, 3)), device="cpu")
    with pytest.raises(ValueError):
        DeviceDataset(X, y, mean=np.zeros((4, 4)), device="cpu")
    ds = DeviceDataset(torch.from_numpy(X), torch.from_numpy(y).long(), device="cpu")
    assert len(ds) == 6 and ds.shape == (6, 4, 4, 3) and ds.mean.dtype == np.float64 and ds.mean.shape == (4, 4, 3)
    assert ds._data.dtype == torch.uint8 and ds._labels.dtype == torch.int32
    assert np.array_equal(ds._labels.numpy(), y)
    with pytest.raises(ValueError):  # no host fallback: the kernel is the only way to a batch
        ds.batch(torch.empty(2, 4, 4, 3), torch.empty(2, dtype=torch.int32))
    with pytest.raises(IndexError):
        ds.upload_index(torch.tensor([0, 6]))
    with pytest.raises(IndexError):
        ds.upload_index(torch.tensor([-1, 2]))
    assert ds.upload_index(torch.tensor([5, 0])).dtype == torch.int32


def test_host_float_is_the_float64_formula():
    X, y, mean = _norm_fixture()
    tr = DeviceDataset(X, y, device="cpu")
    assert np.array_equal(tr.mean, X.astype(np.float64).mean(axis=0))
    want = ((X.astype(np.float64) - mean) / 128).astype(F32)
    assert tr.host_float().dtype == F32 and np.array_equal(tr.host_float(), want)
    Xte, yte = _u8((8, 8, 4), n=9, seed=3)
    te = DeviceDataset(Xte, yte, mean=tr.mean, device="cpu")  # a test set takes the training set's mean
    assert np.array_equal(te.host_float(), ((Xte.astype(np.float64) - mean) / 128).astype(F32))
    fl = DeviceDataset(want, y, device="cpu")  # float data is itself
    assert fl.mean is None and np.array_equal(fl.host_float(), want)
    Xf, yf = _u8((20,), n=11, seed=4)  # [n, F]
    pf = DeviceDataset(Xf, yf, device="cpu")
    assert pf.shape == (11, 20) and pf.mean.shape == (20,)
    assert np.array_equal(pf.host_float(), ((Xf.astype(np.float64) - Xf.astype(np.float64).mean(axis=0)) / 128).astype(F32))


def test_norm_fixture_tells_float64_from_float32_arithmetic():
    """The fixture of the normalisation test is effective: on it the cheaper fp32 formulation differs
    from load_data's float64 one, so a kernel computing in fp32 cannot pass."""
    X, _, mean = _norm_fixture()
    assert set(np.unique(X)) == set(range(256))
    want = _norm(X, mean)
    cheap = (X.astype(F32) - mean.astype(F32)) / F32(128)
    assert cheap.dtype == F32 and np.any(cheap != want)


# ------------------------------------------------------------------------------------ GPU: the kernel
def _buffers(B, shape, offset=False):
    """(X, y) output buffers; offset: X starts 4 bytes past a 16-byte boundary."""
    n = B * int(np.prod(shape))
    buf = torch.full((n + 4,), float("nan"), dtype=torch.float32, device=DEV)
    X = buf[1:1 + n] if offset else buf[:n]
    assert X.data_ptr() % 16 == (4 if offset else 0)
    return X.view((B,) + tuple(shape)), torch.full((B,), -7, dtype=torch.int32, device=DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uint8", "float32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batch_gather_matches_oracle(shape, kind):
    Xu, y = _u8(shape)
    ds = DeviceDataset(Xu, y, device=DEV)
    xn = ds.host_float()
    if kind == "float32":
        ds = DeviceDataset(xn, y, device=DEV)
    idx = torch.tensor(IDX, dtype=torch.int32, device=DEV)
    for pad in (0, 1, 4):  # pad 4 on a 4- or 5-row image: whole rows and columns fall outside
        for flip in (True, False):
            for base in (0, 3):
                want = _oracle(xn[IDX], pad, flip, base)
                for offset in (False, True):
                    oX, oy = _buffers(len(IDX), shape, offset)
                    ds.batch(oX, oy, idx=idx, pad=pad, flip=flip, base=base, seed=SEED, counter=COUNTER)
                    assert np.array_equal(oX.cpu().numpy(), want), (pad, flip, base, offset)
                    assert np.array_equal(oy.cpu().numpy(), y[IDX])


@pytest.mark.gpu
def test_normalisation_is_float64_exact():
    X, y, _ = _norm_fixture()
    ds = DeviceDataset(X, y, device=DEV)
    idx = torch.tensor(IDX, dtype=torch.int32, device=DEV)
    oX, oy = _buffers(len(IDX), X.shape[1:])
    ds.batch(oX, oy, idx=idx)
    assert np.array_equal(oX.cpu().numpy(), ds.host_float()[IDX])
    assert np.array_equal(oX.cpu().numpy(), _norm(X, X.mean(axis=0, dtype=np.float64))[IDX])


@pytest.mark.gpu
@pytest.mark.parametrize("first", [0, 32])  # 32 + 5 == n_data
def test_batch_gather_without_index(first):
    Xu, y = _u8((5, 7, 3))
    ds = DeviceDataset(Xu, y, device=DEV)
    oX, oy = _buffers(5, (5, 7, 3))
    ds.batch(oX, oy, first=first, pad=1, flip=True, seed=SEED, counter=COUNTER)
    assert np.array_equal(oX.cpu().numpy(), _oracle(ds.host_float()[first:first + 5], 1, True, 0))
    assert np.array_equal(oy.cpu().numpy(), y[first:first + 5])
    with pytest.raises(IndexError):
        ds.batch(oX, oy, first=33)
    with pytest.raises(IndexError):  # a caller's idx is range-checked
        ds.batch(oX, oy, idx=torch.tensor([0, 1, 2, 3, 37], dtype=torch.int32, device=DEV))


@pytest.mark.gpu
def test_two_shards_equal_one_batch():
    Xu, y = _u8((8, 8, 3))
    ds = DeviceDataset(Xu, y, device=DEV)
    idx = torch.tensor([3, 36, 0, 11, 11, 20, 5, 1], dtype=torch.int32, device=DEV)
    oX, oy = _buffers(8, (8, 8, 3))
    ds.batch(oX, oy, idx=idx, pad=4, flip=True, seed=SEED, counter=COUNTER)
    for r in (0, 1):
        sX, sy = _buffers(4, (8, 8, 3))
        ds.batch(sX, sy, idx=idx[4 * r:4 * r + 4], pad=4, flip=True, base=4 * r, seed=SEED, counter=COUNTER)
        assert torch.equal(sX, oX[4 * r:4 * r + 4]) and torch.equal(sy, oy[4 * r:4 * r + 4])


@pytest.mark.gpu
def test_equals_augment_kernel_on_the_gathered_batch():
    from lbt_amd.dfxp import ops
    rng = np.random.default_rng(9)
    X = rng.standard_normal((24, 32, 32, 3)).astype(F32)
    y = rng.integers(0, 10, size=24).astype(np.int32)
    ds = DeviceDataset(X, y, device=DEV)
    perm = rng.permutation(24)[:16]
    oX, oy = _buffers(16, (32, 32, 3))
    ds.batch(oX, oy, idx=torch.from_numpy(perm.astype(np.int32)).to(DEV), pad=4, flip=True, seed=SEED, counter=COUNTER)
    want = ops.augment_flip_crop(torch.from_numpy(X[perm]).to(DEV), 4, SEED, COUNTER)
    assert torch.equal(oX, want)
    assert np.array_equal(oy.cpu().numpy(), y[perm])


# ------------------------------------------------------------------------------------ GPU: the Trainer
def _trainer(seed, B, fused=True):
    """As _fused_trainer of tests/test_edge_cases.py (fused=False: the layer-wise model, which binds no inputs)."""
    from lbt_amd.fused import FusedResNet
    from lbt_amd.models import CIFAR10_Resnet20
    from lbt_amd.runtime import DfxpContext
    from lbt_amd.trainer import Trainer
    ctx = DfxpContext(seed=seed)
    gm = CIFAR10_Resnet20(8, weight_decay=2e-4, ctx=ctx)
    return ctx, gm, Trainer(FusedResNet(gm) if fused else gm, lr=1e-2, momentum=0.9, batch_size=B, use_graph=True)


def _cifar_like(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, size=(n, 32, 32, 3), dtype=np.uint8), rng.integers(0, 10, size=n).astype(np.int32))


def _bn_state(tr):
    return [t.cpu().numpy() for bn in tr._bn_layers() for t in (bn.X_mean_running, bn.X_var_running)]


def _assert_same_state(a, b):
    """(ctx, trainer) pairs: parameters, momentum, exponents, counters, noise step, BN running statistics."""
    (ca, ta), (cb, tb) = a, b
    assert torch.equal(ta.flat.w, tb.flat.w) and torch.equal(ta.flat.a, tb.flat.a)
    assert ca.ranges() == cb.ranges() and torch.equal(ca.counts, cb.counts) and torch.equal(ca.step, cb.step)
    assert torch.equal(ca.nelem, cb.nelem)
    for x, y in zip(_bn_state(ta), _bn_state(tb)):
        assert np.array_equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("fused,augment", [(True, True), (True, False), (False, True)],
                         ids=["fused-augment", "fused-plain", "layerwise-augment"])
def test_train_from_device_dataset_equals_host_arrays(fused, augment):
    Xu, y = _cifar_like(40, 31)  # batches of 16, 16, 8
    Xte, yte = _cifar_like(24, 32)
    ds = DeviceDataset(Xu, y, device=DEV)
    ds_te = DeviceDataset(Xte, yte, mean=ds.mean, device=DEV)
    ca, _, ta = _trainer(31, 16, fused)
    cb, _, tb = _trainer(31, 16, fused)
    ta.dataset = ((ds.host_float(), y), (ds_te.host_float(), yte))
    tb.dataset = (ds, ds_te)
    ta.n_epoch = tb.n_epoch = 2
    torch.manual_seed(5)
    ha = ta.train(augment=augment)
    torch.manual_seed(5)
    hb = tb.train(augment=augment)
    torch.cuda.synchronize()
    assert ha == hb and len(hb) == 2
    assert ta.batch_sizes == tb.batch_sizes == [16, 16, 8] and ta.global_step == tb.global_step == 6
    _assert_same_state((ca, ta), (cb, tb))
    if fused:  # fixed batch buffers: one captured graph per batch size
        assert len(tb._gcache) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layerwise"])
def test_evaluate_device_dataset_equals_arrays(fused):
    Xu, y = _cifar_like(50, 41)  # 20, 20, 10
    ds = DeviceDataset(Xu, y, device=DEV)
    Xf = ds.host_float()
    ca, _, ta = _trainer(41, 16, fused)
    cb, _, tb = _trainer(41, 16, fused)
    x0 = torch.from_numpy(Xf[:16]).to(DEV)
    y0 = torch.from_numpy(y[:16]).to(DEV)
    for tr in (ta, tb):  # off the initial state: counters, exponents and running statistics have moved
        tr.step(x0, y0)
    for testing in (False, True):
        ra = ta.evaluate(Xf, y, batch_size=20, testing=testing)
        rb = tb.evaluate(ds, batch_size=20, testing=testing)
        assert ra == rb, testing
        _assert_same_state((ca, ta), (cb, tb))
    for tr in (ta, tb):  # and training goes on the same afterwards
        tr.step(x0, y0)
    _assert_same_state((ca, ta), (cb, tb))
    with pytest.raises(TypeError):
        tb.evaluate(ds, y)


@pytest.mark.gpu
def test_steady_state_epoch_allocates_no_device_memory(monkeypatch):
    """Epoch 2 of a three-epoch train() (epoch 0 captures the graphs, the partial batch's plan at its end
    has those of the full batches captured again in epoch 1) neither changes torch.cuda.memory_allocated()
    nor makes more device allocations than the one the epoch's permutation upload may take: no batch is
    built by the host. The state at each epoch's start is read where train() draws its permutation."""
    Xu, y = _cifar_like(40, 51)
    ds = DeviceDataset(Xu, y, device=DEV)
    _, _, tr = _trainer(51, 16)
    tr.dataset = (ds, None)
    tr.n_epoch = 3
    seen = []
    randperm = torch.randperm

    def recording_randperm(*a, **k):
        seen.append((torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]))
        return randperm(*a, **k)

    monkeypatch.setattr(torch, "randperm", recording_randperm)
    tr.train()
    end = (torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"])
    monkeypatch.undo()
    assert len(seen) == 3 and tr.global_step == 9
    assert end[0] == seen[2][0]
    assert end[1] - seen[2][1] <= 1
