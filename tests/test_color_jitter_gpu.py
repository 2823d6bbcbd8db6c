"""lbt_batch_resized_crop_jitter and ResizedCropDataset(color_jitter=...) on the GPU against the numpy restatement
(tests/color_jitter_oracle.py); every output comparison is np.array_equal. The cases are those of
tests/color_jitter_cases.py (tests/test_color_jitter.py shows they hold all six orders, both clamps, and contrast
first and last): a 12x12x3 store, the smallest shapes at which each path of the launch can go wrong."""
import numpy as np
import pytest
import torch

import color_jitter_cases as J
import color_jitter_oracle as O
import resized_crop_cases as K
import resized_crop_oracle as R
from lbt_amd.data import ResizedCropDataset
from lbt_amd.dfxp import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dataset(size, jitter, shape=J.STORE, n=K.N_DATA, seed=1, **opts):
    X, y = K.u8(shape, n=n, seed=seed)
    return X, y, ResizedCropDataset(X, y, K.MEAN[3], K.STD[3], size, device=DEV, color_jitter=jitter, **opts)


def _buffers(B, shape, offset=False):
    """(X, y) output buffers; offset: X starts 4 bytes past a 16-byte boundary (the 4-byte store path)."""
    n = B * int(np.prod(shape))
    buf = torch.full((n + 4,), float("nan"), dtype=torch.float32, device=DEV)
    X = buf[1:1 + n] if offset else buf[:n]
    assert X.data_ptr() % 16 == (4 if offset else 0)
    return X.view((B,) + tuple(shape)), torch.full((B,), -7, dtype=torch.int32, device=DEV)


def _idx(src):
    return torch.tensor(list(src), dtype=torch.int32, device=DEV)


def _check(ds, X, y, src, size, *, base=0, counter=J.COUNTER, offset=False, idx=True, first=0):
    """One augmenting batch of ds against the oracle."""
    oX, oy = _buffers(len(src), ds.sample_shape, offset)
    ds.batch(oX, oy, idx=_idx(src) if idx else None, first=first, augment=True, base=base, seed=J.SEED, counter=counter,
             check=False)
    want, labels, _ = O.batch(X, y, src, size, R.of_dataset(ds), ds.jitter, base=base, seed=J.SEED, counter=counter)
    assert np.array_equal(oy.cpu().numpy(), labels)
    assert np.array_equal(oX.cpu().numpy(), want), (size, base, offset)
    return oX, oy


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset-4-bytes"])
@pytest.mark.parametrize("size", J.OUTPUTS, ids=lambda s: "%dx%d" % s)
def test_jitter_matches_oracle(size, offset):
    """Six samples at base 0 (all six orders) under the reference's (0.4, 0.4, 0.4)."""
    X, y, ds = _dataset(size, J.FULL)
    _check(ds, X, y, J.SRC, size, offset=offset)


def test_contrast_mean_is_over_the_image_not_the_strip():
    """B = 12 of 97 rows: 49 strips of two rows, the last of one. A mean taken over a strip cannot pass."""
    size = (97, 8)
    assert ops.batch_resized_crop_jitter_work(12, 97) == 12 * 49
    X, y, ds = _dataset(size, J.FULL)
    _check(ds, X, y, J.SRC + J.SRC[::-1], size)
    assert ds._work[12].numel() == 12 * 49


@pytest.mark.parametrize("offset", [False, True], ids=["16-byte", "4-byte"])
def test_rows_of_more_pixels_than_a_workgroup_has_threads(offset):
    """Wo = 348: 87 four-pixel groups per row (two rows in flight, 82 threads idle), or, with X off by one
    float, 348 single pixels against 256 threads (two passes over the row, the second partial)."""
    X, y, ds = _dataset((3, 348), J.FULL, shape=(5, 300, 3), n=4, seed=10)
    _check(ds, X, y, [2, 3, 0], (3, 348), offset=offset)


@pytest.mark.parametrize("jitter", J.PARTIAL, ids=lambda j: "b%s-c%s-s%s" % j)
def test_each_operation_alone_and_contrast_off(jitter):
    for size in ((8, 8), (7, 5)):
        X, y, ds = _dataset(size, jitter)
        _check(ds, X, y, J.SRC, size)
        assert (ds._jitter_work(6) is None) == (jitter[1] == 0)  # contrast off: no statistics pass, no scratch


def test_factors_pinned_to_one_equal_the_plain_launch():
    for size in J.OUTPUTS:
        X, y, plain = _dataset(size, None)
        for jitter in ((0, 0, 0), ((1, 1), (1, 1), (1, 1))):
            ds = ResizedCropDataset(X, y, K.MEAN[3], K.STD[3], size, device=DEV, color_jitter=jitter)
            assert ds.jitter == (4096,) * 6
            for offset in (False, True):
                a, b = _buffers(6, ds.sample_shape, offset), _buffers(6, ds.sample_shape, offset)
                ds.batch(*a, idx=_idx(J.SRC), augment=True, base=3, seed=J.SEED, counter=J.COUNTER)
                plain.batch(*b, idx=_idx(J.SRC), augment=True, base=3, seed=J.SEED, counter=J.COUNTER)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_validation_batches_ignore_the_jitter():
    X, y, ds = _dataset((8, 8), J.FULL)
    _, _, plain = _dataset((8, 8), None)
    for kw in (dict(idx=_idx(J.SRC)), dict(first=31)):
        a, b = _buffers(6, ds.sample_shape), _buffers(6, ds.sample_shape)
        ds.batch(*a, augment=False, seed=J.SEED, counter=J.COUNTER, **kw)
        plain.batch(*b, augment=False, seed=J.SEED, counter=J.COUNTER, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = _buffers(6, ds.sample_shape), _buffers(6, ds.sample_shape)
    ds.test_batch(*a, first=2)
    plain.test_batch(*b, first=2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    want, labels, _ = R.batch(X, y, range(2, 8), (8, 8), R.of_dataset(ds), center=ds.center)
    assert np.array_equal(a[0].cpu().numpy(), want) and np.array_equal(a[1].cpu().numpy(), labels)
    # the entry point itself with augment = 0: jitter bounds and scratch are ignored
    c = _buffers(6, ds.sample_shape)
    ops.batch_resized_crop_jitter(ds._data, ds._labels, c[0], c[1], ds._ratio, ds._shift, ds._scale, a_lo=ds.a_lo,
                                  a_hi=ds.a_hi, q_lo=ds.q_lo, q_hi=ds.q_hi, center=ds.center, jitter=ds.jitter, work=None,
                                  first=2, augment=False)
    assert torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])


def test_two_shards_equal_one_batch():
    X, y, ds = _dataset((8, 8), J.FULL)
    src = J.SRC + [3, 11, 11, 20, 5, 1]
    oX, oy = _check(ds, X, y, src, (8, 8))
    for r in (0, 1):
        sX, sy = _check(ds, X, y, src[6 * r:6 * r + 6], (8, 8), base=6 * r)
        assert torch.equal(sX, oX[6 * r:6 * r + 6]) and torch.equal(sy, oy[6 * r:6 * r + 6])


def test_out_of_range_index_gives_zeros_and_minus_one():
    X, y, ds = _dataset((8, 8), J.FULL)
    src = [4, 37, -1, 36, 1 << 20, 0]
    oX, oy = _check(ds, X, y, src, (8, 8))
    got = oX.cpu().numpy()
    assert oy.tolist() == [y[4], -1, -1, y[36], -1, y[0]]
    assert not got[1].any() and not got[2].any() and not got[4].any() and got[0].any() and got[3].any() and got[5].any()


@pytest.mark.parametrize("first", [0, 31])  # 31 + 6 == n_data
def test_jitter_without_index(first):
    X, y, ds = _dataset((7, 5), J.FULL)
    _check(ds, X, y, list(range(first, first + 6)), (7, 5), idx=False, first=first)
    oX, oy = _buffers(6, ds.sample_shape)
    with pytest.raises(IndexError):
        ds.batch(oX, oy, first=32, augment=True)


def test_scratch_is_reused_with_nothing_left_over():
    """Two launches in a row on the same scratch, other counters (other orders, factors and means): each equals
    its oracle. Then a scratch overwritten beforehand changes nothing: every entry is written before read."""
    X, y, ds = _dataset((16, 16), J.FULL)
    a, _ = _check(ds, X, y, J.SRC, (16, 16), counter=J.COUNTER)
    work = ds._work[6]
    b, _ = _check(ds, X, y, J.SRC, (16, 16), counter=J.COUNTER + 1)
    assert ds._work[6] is work and len(ds._work) == 1 and not torch.equal(a, b)
    work.fill_(-1)
    c, _ = _check(ds, X, y, J.SRC, (16, 16), counter=J.COUNTER)
    assert torch.equal(a, c)


def test_ops_checks_scratch_and_bounds():
    X, y, ds = _dataset((8, 8), J.FULL)
    oX, oy = _buffers(6, ds.sample_shape)
    kw = dict(a_lo=ds.a_lo, a_hi=ds.a_hi, q_lo=ds.q_lo, q_hi=ds.q_hi, center=ds.center, idx=_idx(J.SRC), augment=True)
    args = (ds._data, ds._labels, oX, oy, ds._ratio, ds._shift, ds._scale)
    need = ops.batch_resized_crop_jitter_work(6, 8)
    assert need == 6 * 8
    for bad in (dict(jitter=ds.jitter, work=None), dict(jitter=ds.jitter, work=torch.empty(need - 1, dtype=torch.int64, device=DEV)),
                dict(jitter=ds.jitter, work=torch.empty(need, dtype=torch.int32, device=DEV)),
                dict(jitter=ds.jitter, work=torch.empty(need, dtype=torch.int64)),
                dict(jitter=(5734, 2458) * 3, work=torch.empty(need, dtype=torch.int64, device=DEV)),
                dict(jitter=ds.jitter[:4], work=None)):
        with pytest.raises(ValueError):
            ops.batch_resized_crop_jitter(*args, **kw, **bad)
    assert torch.isnan(oX).all()  # nothing was launched


def test_captured_launch_pair_replays_to_the_eager_result():
    X, y, ds = _dataset((16, 16), J.FULL)
    idx = _idx(J.SRC)
    eager, ey = _check(ds, X, y, J.SRC, (16, 16))
    oX, oy = _buffers(6, ds.sample_shape)
    torch.cuda.synchronize()  # (the eager launch loaded the code objects and allocated the scratch)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ds.batch(oX, oy, idx=idx, augment=True, seed=J.SEED, counter=J.COUNTER, check=False)
    for _ in range(2):
        oX.fill_(float("nan"))
        oy.fill_(-7)
        ds._work[6].fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(oX, eager) and torch.equal(oy, ey)


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


def test_train_epoch_with_color_jitter_equals_hand_loop():
    """One epoch of train() from a jittering dataset (48 images stored 40x40, 32x32 batches of 16) against a
    hand loop over ds.batch(augment=True, base=0, seed=ctx.seed, counter=global_step) + step(): the same
    parameters, momentum, exponents, counters and BN statistics bit for bit, and the same test accuracy. The
    first hand-made batch is also the oracle's, and differs from the batch without jitter."""
    m, s = K.MEAN[3], K.STD[3]
    X, y = K.u8((40, 40, 3), n=48, seed=61)
    Xte, yte = K.u8((40, 40, 3), n=24, seed=62)
    ds = ResizedCropDataset(X, y, m, s, 32, device=DEV, color_jitter=J.FULL)
    ds_te = ResizedCropDataset(Xte, yte, m, s, 32, device=DEV, color_jitter=J.FULL)
    ca, ta = _trainer(61, 16)
    cb, tb = _trainer(61, 16)
    tb.dataset = (ds, ds_te)
    tb.n_epoch = 1
    torch.manual_seed(7)
    hist = tb.train(augment=True)
    torch.manual_seed(7)
    ta.get_train_op()
    perm = torch.randperm(48)
    dperm = ds.upload_index(perm)
    xb = torch.empty((16, 32, 32, 3), dtype=torch.float32, device=DEV)
    yb = torch.empty(16, dtype=torch.int32, device=DEV)
    for b in range(0, 48, 16):
        ds.batch(xb, yb, idx=dperm[b:b + 16], augment=True, base=0, seed=ca.seed, counter=ta.global_step, check=False)
        if b == 0:
            want, labels, _ = O.batch(X, y, perm[:16].tolist(), (32, 32), R.of_dataset(ds), ds.jitter, seed=ca.seed,
                                      counter=ta.global_step)
            plain, _, _ = R.batch(X, y, perm[:16].tolist(), (32, 32), R.of_dataset(ds), augment=True, seed=ca.seed,
                                  counter=ta.global_step)
            assert np.array_equal(xb.cpu().numpy(), want) and np.array_equal(yb.cpu().numpy(), labels)
            assert np.any(want != plain)
        ta.step(xb, yb)
    xte, lte, _ = R.batch(Xte, yte, range(24), (32, 32), R.of_dataset(ds_te), center=ds_te.center)  # never jittered
    acc, _ = ta.evaluate(xte, lte)
    torch.cuda.synchronize()
    assert hist == [acc] and ta.global_step == tb.global_step == 3 and tb.batch_sizes == [16, 16, 16]
    assert torch.equal(ta.flat.w, tb.flat.w) and torch.equal(ta.flat.a, tb.flat.a)
    assert ca.ranges() == cb.ranges() and torch.equal(ca.counts, cb.counts) and torch.equal(ca.step, cb.step)
    assert torch.equal(ca.nelem, cb.nelem)
    for u, v in zip(_bn_state(ta), _bn_state(tb)):
        assert np.array_equal(u, v)
    assert tb.evaluate(ds_te, testing=True) == ta.evaluate(xte, lte, testing=True)
