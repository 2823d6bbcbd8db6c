"""The ImageNet input transform without a GPU (lbt_batch_resized_crop's host checks, ResizedCropDataset's
constructor, and the numpy restatement tests/resized_crop_oracle.py that the GPU tests compare with)."""
import ctypes

import numpy as np
import pytest
import torch

import resized_crop_cases as K
import resized_crop_oracle as R
from lbt_amd import _lib
from lbt_amd.data import DEVICE_DATASETS, DeviceDataset, ResizedCropDataset

F32 = np.float32


# ------------------------------------------------------------------------------------ host checks
ARGS = ("data", "labels", "n_data", "idx", "first", "X", "y", "B", "Hs", "Ws", "C", "Ho", "Wo", "augment", "a_lo", "a_hi",
        "ratio", "q_lo", "q_hi", "ch", "cw", "shift", "scale_c", "base", "seed", "counter")


def _crop_args(**over):
    """A full argument list of lbt_batch_resized_crop with fake non-NULL pointers (never dereferenced: every
    case below is rejected on the host first)."""
    p = ctypes.c_void_p(0x1000)
    a = dict(data=p, labels=p, n_data=37, idx=None, first=0, X=p, y=p, B=5, Hs=12, Ws=10, C=3, Ho=8, Wo=8, augment=1,
             a_lo=10, a_hi=120, ratio=p, q_lo=49152, q_hi=87381, ch=11, cw=9, shift=p, scale_c=p, base=0, seed=1,
             counter=2)
    a.update(over)
    return [a[k] for k in ARGS] + [None]


EINVAL_CASES = [dict(data=None), dict(labels=None), dict(X=None), dict(y=None), dict(ratio=None), dict(shift=None),
                dict(scale_c=None), dict(B=0), dict(B=-1), dict(Hs=0), dict(Ws=0), dict(C=0), dict(C=-3), dict(Ho=0),
                dict(Wo=-1), dict(n_data=0), dict(n_data=-5),
                dict(Hs=8193, a_hi=120), dict(Ws=8193), dict(Ho=8193), dict(Wo=8193),
                dict(Hs=8192, Ws=8192, C=32, ch=1, cw=1), dict(Ho=8192, Wo=8192, C=32),
                dict(a_lo=0), dict(a_lo=-1), dict(a_lo=50, a_hi=49), dict(a_hi=121),
                dict(q_lo=0), dict(q_lo=-1), dict(q_lo=87382), dict(q_hi=1 << 32),
                dict(ch=0), dict(ch=13), dict(cw=0), dict(cw=11), dict(augment=0, ch=13),
                dict(base=-1), dict(base=(1 << 32) - 4), dict(base=1 << 40),
                dict(first=-1), dict(first=33), dict(first=1 << 40)]


@pytest.mark.parametrize("over", EINVAL_CASES, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_resized_crop_host_checks_return_einval(over):
    assert _lib.load().lbt_batch_resized_crop(*_crop_args(**over)) == 1001


# ------------------------------------------------------------------------------------ the dataset class
def test_resized_crop_dataset_argument_checks():
    X, y = K.u8((6, 8, 3), n=6)
    m, s = K.MEAN[3], K.STD[3]
    for bad in (X.astype(np.int16), X.astype(F32)):
        with pytest.raises(TypeError):
            ResizedCropDataset(bad, y, m, s, 4, device="cpu")
    with pytest.raises(TypeError):
        ResizedCropDataset(X, y.astype(F32), m, s, 4, device="cpu")
    for kw in (dict(y=y[:5]), dict(X=X[:, :, :, 0]), dict(mean=m[:2]), dict(std=(0.2, 0.0, 0.2)), dict(size=0),
               dict(size=(4, 8193)), dict(scale=(0.0, 1.0)), dict(scale=(0.5, 0.4)), dict(scale=(0.5, 1.5)),
               dict(ratio=(0.0, 1.0)), dict(ratio=(2.0, 1.0)), dict(ratio=(1.0, 70000.0)), dict(center=(7, 8)),
               dict(center=(6, 0))):
        a = dict(X=X, y=y, mean=m, std=s, size=4)
        a.update(kw)
        with pytest.raises(ValueError):
            ResizedCropDataset(device="cpu", **a)
    ds = ResizedCropDataset(torch.from_numpy(X), torch.from_numpy(y).long(), m, s, (4, 5), device="cpu")
    assert isinstance(ds, DEVICE_DATASETS) and len(ds) == 6 and ds.shape == (6, 6, 8, 3) and ds.sample_shape == (4, 5, 3)
    assert ds.center == (5, 7) and ds._data.dtype == torch.uint8 and ds._labels.dtype == torch.int32
    assert ResizedCropDataset(np.zeros((2, 256, 256, 3), np.uint8), y[:2], m, s, 224, device="cpu").center == (224, 224)
    with pytest.raises(ValueError):  # no host fallback: the kernel is the only way to a batch
        ds.batch(torch.empty(2, 4, 5, 3), torch.empty(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        ds.batch(torch.empty(2, 6, 8, 3), torch.empty(2, dtype=torch.int32))
    with pytest.raises(IndexError):
        ds.upload_index(torch.tensor([0, 6]))
    assert ds.upload_index(torch.tensor([5, 0])).dtype == torch.int32


def test_dataset_constants_are_the_oracles():
    X, y = K.u8((256, 256, 3), n=2)
    ds = ResizedCropDataset(X, y, K.MEAN[3], K.STD[3], 224, device="cpu")
    k = R.constants(256, 256, K.MEAN[3], K.STD[3])
    assert (ds.a_lo, ds.a_hi, ds.q_lo, ds.q_hi) == (5243, 65536, 49152, 87381) == (k["a_lo"], k["a_hi"], k["q_lo"], k["q_hi"])
    assert ds.ratio_q16.dtype == np.uint32 and ds.ratio_q16.shape == (256,) and np.array_equal(ds.ratio_q16, k["ratio_q16"])
    assert np.all(np.diff(ds.ratio_q16.astype(np.int64)) > 0) and ds.q_lo < ds.ratio_q16[0] and ds.ratio_q16[-1] < ds.q_hi
    assert np.array_equal(ds._ratio.numpy().view(np.uint32), ds.ratio_q16)
    for name in ("shift", "scale_c"):
        assert getattr(ds, name).dtype == np.float64 and np.array_equal(getattr(ds, name), k[name])
    assert np.array_equal(ds.shift, 65536.0 * 255.0 * np.array(K.MEAN[3]))
    assert all(np.array_equal(R.of_dataset(ds)[n], k[n]) for n in k)
    tiny = ResizedCropDataset(X[:, :1, :1], y, K.MEAN[3], K.STD[3], 1, device="cpu")  # a one-pixel area range
    assert (tiny.a_lo, tiny.a_hi, tiny.center) == (1, 1, (1, 1))


def test_both_dataset_classes_share_the_trainers_surface():
    X, y = K.u8((6, 8, 3), n=6)
    a = DeviceDataset(X, y, device="cpu")
    b = ResizedCropDataset(X, y, K.MEAN[3], K.STD[3], 4, device="cpu")
    assert a.sample_shape == (6, 8, 3) and b.sample_shape == (4, 4, 3)
    assert DeviceDataset(X.reshape(6, -1), y, device="cpu").sample_shape == (144,)
    for ds in (a, b):
        assert callable(ds.train_batch) and callable(ds.test_batch) and callable(ds.upload_index) and len(ds) == 6


# ------------------------------------------------------------------------------------ the oracle
def _fixture():
    """A 16x16x3 image holding all 256 values in every channel (each channel another order), and a box,
    off the pixel grid in both directions, resampled to 11x13."""
    rng = np.random.default_rng(2)
    img = np.stack([rng.permutation(256) for _ in range(3)], axis=1).reshape(16, 16, 3).astype(np.uint8)
    return img, (1, 2, 13, 11, 0), (11, 13), R.constants(16, 16, K.MEAN[3], K.STD[3])


def test_identity_box_is_the_plain_normalisation():
    img, _, _, k = _fixture()
    want = ((img.astype(np.float64) * 65536 - k["shift"]) * k["scale_c"]).astype(F32)
    got, labels, boxes = R.batch(img[None], np.array([4], np.int32), [0], (16, 16), k, center=(16, 16))
    assert boxes == [(0, 0, 16, 16, -1)] and labels[0] == 4
    assert got.dtype == F32 and np.array_equal(got[0], want)
    assert np.array_equal(R.resample(img, (3, 5, 7, 9, 0), False, 7, 9, k), want[3:10, 5:14])  # an inner box
    assert np.array_equal(R.resample(img, (3, 5, 7, 9, 0), True, 7, 9, k), want[3:10, 5:14][:, ::-1])
    torch_like = ((img.astype(np.float64) / 255 - np.array(K.MEAN[3])) / np.array(K.STD[3]))  # Normalize's formula
    assert np.allclose(want, torch_like, rtol=1e-6, atol=1e-6)


def test_fixture_tells_the_cheaper_formulations_apart():
    """On the fixture the oracle differs from the same transform normalised in fp32, and from fy / fx
    truncated instead of rounded: a kernel doing either cannot pass."""
    img, box, (Ho, Wo), k = _fixture()
    assert all(set(np.unique(img[:, :, c])) == set(range(256)) for c in range(3))
    want = R.resample(img, box, False, Ho, Wo, k)
    f32 = R.resample(img, box, False, Ho, Wo, k, norm="f32")
    trunc = R.resample(img, box, False, Ho, Wo, k, frac="trunc")
    assert want.dtype == f32.dtype == trunc.dtype == F32
    assert np.any(f32 != want) and np.any(trunc != want)
    assert np.allclose(f32, want, rtol=1e-5, atol=1e-5) and np.abs(trunc - want).max() < 0.1  # the same transform
    ident = (0, 0, 16, 16, 0)  # and the fp32 formulation already differs with no resampling at all
    assert np.any(R.resample(img, ident, False, 16, 16, k, norm="f32") != R.resample(img, ident, False, 16, 16, k))


def test_taps_are_half_pixel_bilinear():
    for inn, out in ((13, 11), (5, 16), (1, 4), (7, 7), (224, 224), (256, 224)):
        p0, p1, f = R.taps(inn, out)
        pos = np.clip((np.arange(out) + 0.5) * inn / out - 0.5, 0, inn - 1)  # where the sample lies
        assert np.all(np.abs(p0 + f / 256 - pos) <= 1 / 512 + 1e-12)
        assert np.all((0 <= p0) & (p0 <= p1) & (p1 <= inn - 1) & (p1 - p0 <= 1) & (0 <= f) & (f <= 256))
        assert np.all((f == 0) | (p1 == p0 + 1))  # a weight on the upper tap only where there is one


def test_boxes_of_4096_draws_lie_inside_a_256_store():
    k = R.constants(256, 256, K.MEAN[3], K.STD[3])
    boxes = [R.random_box(n, 256, 256, k, K.SEED, K.COUNTER) for n in range(4096)]
    for top, left, h, w, t in boxes:
        assert 1 <= h <= 256 and 1 <= w <= 256 and 0 <= top <= 256 - h and 0 <= left <= 256 - w
        assert k["a_lo"] * 0.7 <= h * w <= k["a_hi"] * 1.05 and 0.7 <= w / h <= 1.45
    attempts = np.array([b[4] for b in boxes])
    assert np.any(attempts > 0) and np.mean(attempts == 0) > 0.5
    areas = np.array([b[2] * b[3] for b in boxes]) / 65536.0
    assert areas.min() < 0.1 and areas.max() > 0.7  # the whole scale range is drawn from
    assert 0.4 < np.mean([R.flips(n, K.SEED, K.COUNTER) for n in range(512)]) < 0.6


def test_gpu_case_list_covers_every_path():
    """First-attempt accept, later accept, and the fallback's wide, tall and whole-image branches all occur
    among the boxes the GPU test's cases draw (samples base .. base + 4 of each store)."""
    seen = set()
    for (Hs, Ws, C), opts in K.STORES:
        k = R.constants(Hs, Ws, K.MEAN[C], K.STD[C], **opts)
        for n in range(max(K.BASES) + len(K.IDX)):
            top, left, h, w, t = R.random_box(n, Hs, Ws, k, K.SEED, K.COUNTER)
            if t == 0:
                seen.add("first")
            elif t < R.FALLBACK:
                seen.add("later")
            elif Ws * 65536 > k["q_hi"] * Hs:
                assert h == Hs and w < Ws and left == (Ws - w) // 2
                seen.add("wide")
            elif Ws * 65536 < k["q_lo"] * Hs:
                assert w == Ws and h < Hs and top == (Hs - h) // 2
                seen.add("tall")
            else:
                assert (top, left, h, w) == (0, 0, Hs, Ws)
                seen.add("whole")
    assert seen == {"first", "later", "wide", "tall", "whole"}
    pinned = R.constants(12, 12, K.MEAN[3], K.STD[3], scale=(1.0, 1.0), ratio=(1.0, 1.0))
    assert R.random_box(0, 12, 12, pinned, K.SEED, K.COUNTER) == (0, 0, 12, 12, 0)
    for shape, opts in (((4, 40, 3), K.STORES[2][1]), ((40, 4, 1), K.STORES[3][1])):  # every sample falls back
        k = R.constants(shape[0], shape[1], K.MEAN[shape[2]], K.STD[shape[2]], **opts)
        assert all(R.random_box(n, shape[0], shape[1], k, K.SEED, K.COUNTER)[4] == R.FALLBACK for n in range(8))
