"""lbt_batch_ragged_crop, lbt_batch_ragged_crop_jitter and RaggedCropDataset on the GPU against the numpy
restatement (tests/ragged_crop_oracle.py, which composes the uniform oracles per sample); every comparison is
np.array_equal or torch.equal. The cases are those of tests/ragged_crop_cases.py (tests/test_ragged_crop.py
shows they reach every path of the box computation): the smallest stores at which a kernel that reads one
sample's geometry for another, or draws a box from the wrong area range, cannot pass."""
import numpy as np
import pytest
import torch

import ragged_crop_cases as G
import ragged_crop_oracle as RG
import resized_crop_cases as K
from lbt_amd.data import RaggedCropDataset, ResizedCropDataset

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FULL = (0.4, 0.4, 0.4)  # the reference's ColorJitter
KEY = dict(seed=G.SEED, counter=G.COUNTER)


def _ds(images, y, size, **opts):
    return RaggedCropDataset(images, y, G.MEAN, G.STD, size, device=DEV, **opts)


def _buffers(B, shape, offset=False):
    """(X, y) output buffers; offset: X starts 4 bytes past a 16-byte boundary."""
    n = B * int(np.prod(shape))
    buf = torch.full((n + 4,), float("nan"), dtype=torch.float32, device=DEV)
    X = buf[1:1 + n] if offset else buf[:n]
    assert X.data_ptr() % 16 == (4 if offset else 0)
    return X.view((B,) + tuple(shape)), torch.full((B,), -7, dtype=torch.int32, device=DEV)


def _idx(src):
    return torch.tensor(list(src), dtype=torch.int32, device=DEV)


def _check(ds, images, y, src, size, *, augment=True, base=0, offset=False, opts={}, idx=True, first=0, check=True):
    """One batch of ds against the ragged oracle (with ds's jitter bounds when it jitters)."""
    oX, oy = _buffers(len(src), ds.sample_shape, offset)
    ds.batch(oX, oy, idx=_idx(src) if idx else None, first=first, augment=augment, base=base, check=check, **KEY)
    want, labels, _ = RG.batch(images, y, src, size, G.MEAN, G.STD, augment=augment, center=ds.center, jitter=ds.jitter,
                               base=base, **KEY, **opts)
    assert np.array_equal(oy.cpu().numpy(), labels), (size, augment, base, offset)
    assert np.array_equal(oX.cpu().numpy(), want), (size, augment, base, offset)
    return oX, oy


# ------------------------------------------------------------------------------------ 1, 2: the mixed store
@pytest.mark.parametrize("opts", G.OPTION_SETS, ids=G.OPTION_IDS)
def test_mixed_store_matches_oracle(opts):
    images, y = G.store()
    for size in G.OUTPUTS:
        ds = _ds(images, y, size, **opts)
        for augment in (True, False):
            for base in G.BASES:
                for offset in (False, True):
                    _check(ds, images, y, G.IDX, size, augment=augment, base=base, offset=offset, opts=opts)


@pytest.mark.parametrize("opts", G.OPTION_SETS, ids=G.OPTION_IDS)
@pytest.mark.parametrize("jitter", [FULL, (0.4, 0, 0.4)], ids=["full", "contrast-off"])
def test_mixed_store_with_jitter_matches_oracle(jitter, opts):
    """Six samples at base 0: keys 0..5 draw the six orders (tests/test_color_jitter.py). (8,8) and (16,16): four
    pixels per lane when X is aligned; (7,5), (1,1) and every offset X: one."""
    images, y = G.store()
    for size in G.OUTPUTS:
        ds = _ds(images, y, size, color_jitter=jitter, **opts)
        assert (ds._jitter_work(6) is None) == (jitter[1] == 0)  # contrast off: no statistics pass, work=None
        for offset in (False, True):
            _check(ds, images, y, G.IDX[:6], size, offset=offset, opts=opts)
    plain = _ds(images, y, (8, 8), **opts)
    a, _ = _check(plain, images, y, G.IDX[:6], (8, 8), opts=opts)
    b, _ = _check(_ds(images, y, (8, 8), color_jitter=jitter, **opts), images, y, G.IDX[:6], (8, 8), opts=opts)
    assert not torch.equal(a, b)


# ------------------------------------------------------------------------------------ 3: against the uniform launch
def test_equal_images_equal_the_uniform_dataset():
    X, y = K.u8((9, 14, 3))
    for jitter in (None, FULL):
        uni = ResizedCropDataset(X, y, G.MEAN, G.STD, (8, 8), device=DEV, color_jitter=jitter)
        rag = _ds(list(X), y, (8, 8), center=uni.center, color_jitter=jitter)
        for augment in (True, False):
            for base in G.BASES:
                a, b = _buffers(10, (8, 8, 3)), _buffers(10, (8, 8, 3))
                uni.batch(*a, idx=_idx(G.IDX), augment=augment, base=base, **KEY)
                rag.batch(*b, idx=_idx(G.IDX), augment=augment, base=base, **KEY)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
                assert not torch.isnan(a[0]).any()


# ------------------------------------------------------------------------------------ 4: the reference's validation
def test_identity_validation_is_the_central_pixels():
    """Images no smaller than the output with the centre box the output's size: the resample is the identity and
    a validation batch is the image's central pixels, normalised -- Resize(256) + CenterCrop(224) on a store of
    short side 256, at a sixteenth of the size."""
    shapes = [(16, 16), (20, 16), (16, 31), (33, 16), (16, 24)]  # short side 16
    images, y = G.store(n=5, seed=4, shapes=shapes)
    ds = _ds(images, y, 16, center=(16, 16))
    oX, oy = _buffers(5, (16, 16, 3))
    ds.batch(oX, oy)
    got = oX.cpu().numpy()
    for s, (im, (H, W)) in enumerate(zip(images, shapes)):
        mid = im[(H - 16) // 2:(H - 16) // 2 + 16, (W - 16) // 2:(W - 16) // 2 + 16].astype(np.float64)
        assert np.array_equal(got[s], ((mid * 65536 - ds.shift) * ds.scale_c).astype(np.float32)), s
    assert np.array_equal(oy.cpu().numpy(), y)
    short16 = _ds(images, y, 14)  # center=None: the square of 7/8 of the short side, 14 of 16 in every image
    assert [int(v) for v in short16.geom["ch"]] == [14] * 5 == [int(v) for v in short16.geom["cw"]]
    oX, oy = _buffers(5, (14, 14, 3))
    short16.test_batch(oX, oy, first=0)
    got = oX.cpu().numpy()
    for s, (im, (H, W)) in enumerate(zip(images, shapes)):
        mid = im[(H - 14) // 2:(H - 14) // 2 + 14, (W - 14) // 2:(W - 14) // 2 + 14].astype(np.float64)
        assert np.array_equal(got[s], ((mid * 65536 - ds.shift) * ds.scale_c).astype(np.float32)), s


# ------------------------------------------------------------------------------------ 5 - 7: the launch's shapes
def test_rows_split_into_strips_equal_the_oracle():
    """Few samples of many rows: the launch cuts every sample into strips of rows (one row each here)."""
    images, y = G.store(n=6, seed=8, shapes=[(40, 36), (30, 50), (44, 28), (36, 36), (52, 21), (25, 47)])
    for jitter in (None, FULL):
        ds = _ds(images, y, (48, 20), color_jitter=jitter)
        for augment in (True, False):
            _check(ds, images, y, [5, 0, 3], (48, 20), augment=augment)


@pytest.mark.parametrize("B", [300, 1100])  # strips of 3, 3, 3 and 1 rows; one strip of all 10 rows
def test_many_samples_take_strips_of_several_rows(B):
    shapes = [(6, 7), (5, 5), (9, 4), (3, 11), (8, 8), (7, 6), (4, 4), (10, 3), (2, 9)]
    images, y = G.store(n=9, seed=9, shapes=shapes)
    src = np.random.default_rng(B).integers(0, 9, size=B)
    ds = _ds(images, y, (10, 4))
    _check(ds, images, y, src.tolist(), (10, 4), check=False)


@pytest.mark.parametrize("offset", [False, True], ids=["16-byte", "4-byte"])
def test_rows_of_more_stores_than_a_workgroup_has_threads(offset):
    """Wo*C = 1044: 261 16-byte stores or 1044 4-byte stores per row against 256 threads (several passes over
    the row, the last one partial); with jitter 87 four-pixel groups, or 348 single pixels."""
    images, y = G.store(n=4, seed=10, shapes=[(5, 300), (4, 310), (7, 290), (5, 301)])
    for jitter in (None, FULL):
        ds = _ds(images, y, (3, 348), color_jitter=jitter)
        for augment in (True, False):
            _check(ds, images, y, [2, 3, 0], (3, 348), augment=augment, offset=offset)


# ------------------------------------------------------------------------------------ 8 - 10: shards, first, range
def test_two_shards_equal_one_batch():
    images, y = G.store()
    src = [3, 36, 0, 11, 11, 20, 5, 1]
    for jitter in (None, FULL):
        ds = _ds(images, y, (8, 8), color_jitter=jitter)
        oX, oy = _check(ds, images, y, src, (8, 8))
        for r in (0, 1):
            sX, sy = _check(ds, images, y, src[4 * r:4 * r + 4], (8, 8), base=4 * r)
            assert torch.equal(sX, oX[4 * r:4 * r + 4]) and torch.equal(sy, oy[4 * r:4 * r + 4])


@pytest.mark.parametrize("first", [0, 32])  # 32 + 5 == n_data
def test_ragged_crop_without_index(first):
    images, y = G.store()
    ds = _ds(images, y, (7, 5))
    for augment in (True, False):
        _check(ds, images, y, list(range(first, first + 5)), (7, 5), augment=augment, idx=False, first=first)
    oX, oy = _buffers(5, (7, 5, 3))
    with pytest.raises(IndexError):
        ds.batch(oX, oy, first=33)
    with pytest.raises(IndexError):
        ds.batch(oX, oy, first=-1)
    with pytest.raises(IndexError):  # a caller's idx is range-checked
        ds.batch(oX, oy, idx=_idx([0, 1, 2, 3, 37]))
    assert torch.isnan(oX).all()  # nothing was launched


def test_out_of_range_index_gives_zeros_and_minus_one():
    images, y = G.store()
    src = [4, 37, -1, 36, 1 << 20, 0]
    for jitter in (None, FULL):
        ds = _ds(images, y, (8, 8), color_jitter=jitter)
        for augment in (True, False):
            oX, oy = _check(ds, images, y, src, (8, 8), augment=augment, check=False)
            got = oX.cpu().numpy()
            assert oy.tolist() == [y[4], -1, -1, y[36], -1, y[0]]
            assert not got[1].any() and not got[2].any() and not got[4].any() and got[0].any() and got[3].any()


def test_captured_launches_replay_to_the_eager_result():
    """Stream-ordered, allocation-free: the plain launch and the jitter's pair captured into one graph."""
    images, y = G.store()
    plain, jit = _ds(images, y, (16, 16)), _ds(images, y, (16, 16), color_jitter=FULL)
    idx = _idx(G.IDX)
    eager = [_check(ds, images, y, G.IDX, (16, 16)) for ds in (plain, jit)]
    outs = [_buffers(10, (16, 16, 3)) for _ in range(2)]
    torch.cuda.synchronize()  # (the eager launches loaded the code objects and allocated the scratch)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for ds, (oX, oy) in zip((plain, jit), outs):
            ds.batch(oX, oy, idx=idx, augment=True, check=False, **KEY)
    for _ in range(2):
        for oX, oy in outs:
            oX.fill_(float("nan"))
            oy.fill_(-7)
        jit._work[10].fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        for (oX, oy), (eX, ey) in zip(outs, eager):
            assert torch.equal(oX, eX) and torch.equal(oy, ey)


# ------------------------------------------------------------------------------------ 11: the Trainer
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


def _sides(n, seed):
    rng = np.random.default_rng(seed)
    return [tuple(int(v) for v in rng.integers(36, 45, size=2)) for _ in range(n)]


def test_train_epoch_from_ragged_dataset_equals_hand_loop():
    """One epoch of train() (48 images with sides in 36..44, 32x32 batches of 16) and its evaluate() against a
    hand loop that builds every batch with the ragged oracle and calls step(): the same parameters, momentum,
    exponents, counters and BN statistics bit for bit, and the same test accuracy."""
    shapes, shapes_te = _sides(48, 63), _sides(24, 64)
    assert len(set(shapes)) > 20 and min(min(s) for s in shapes) >= 36 and max(max(s) for s in shapes) <= 44
    images, y = G.store(n=48, seed=61, shapes=shapes)
    images_te, yte = G.store(n=24, seed=62, shapes=shapes_te)
    ds, ds_te = _ds(images, y, 32), _ds(images_te, yte, 32)
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
        xb, yb, _ = RG.batch(images, y, perm[b:b + 16], (32, 32), G.MEAN, G.STD, augment=True, seed=ca.seed,
                             counter=ta.global_step)
        ta.step(torch.from_numpy(xb).to(DEV), torch.from_numpy(yb).to(DEV))
    xte, lte, _ = RG.batch(images_te, yte, range(24), (32, 32), G.MEAN, G.STD)
    acc, _ = ta.evaluate(xte, lte)
    torch.cuda.synchronize()
    assert hist == [acc] and ta.global_step == tb.global_step == 3 and tb.batch_sizes == [16, 16, 16]
    assert torch.equal(ta.flat.w, tb.flat.w) and torch.equal(ta.flat.a, tb.flat.a)
    assert ca.ranges() == cb.ranges() and torch.equal(ca.counts, cb.counts) and torch.equal(ca.step, cb.step)
    assert torch.equal(ca.nelem, cb.nelem)
    for u, v in zip(_bn_state(ta), _bn_state(tb)):
        assert np.array_equal(u, v)
    assert tb.evaluate(ds_te, testing=True) == ta.evaluate(xte, lte, testing=True)
