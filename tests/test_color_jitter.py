"""Colour jitter in the ImageNet input launch without a GPU: the integer definition's known answers, the numpy
restatement (tests/color_jitter_oracle.py) against the same formulas in float64, the reach of the GPU test's
cases, lbt_batch_resized_crop_jitter's host checks and ResizedCropDataset's constructor."""
import ctypes

import numpy as np
import pytest

import color_jitter_cases as J
import color_jitter_oracle as O
import resized_crop_cases as K
import resized_crop_oracle as R
from lbt_amd import _lib
from lbt_amd.data import ResizedCropDataset

T = 255 * 65536


# ------------------------------------------------------------------------------------ known answers
def test_grey_blend_and_mean_by_hand():
    assert O.T == T and O.ONE == 4096 and sum(O.GREY) == 65536
    # grey: (19595 + 2 * 38470 + 3 * 7471 + 32768) >> 16 = 151716 >> 16; (3 * 19595 + 32768) >> 16 = 91553 >> 16
    assert O.grey(np.array([1, 2, 3], dtype=np.int64)) == 2
    assert O.grey(np.array([3, 0, 0], dtype=np.int64)) == 1
    assert O.grey(np.array([T, T, T], dtype=np.int64)) == T  # the weights sum to 65536: grey <= T
    assert O.grey(np.array([10 << 16, 20 << 16, 30 << 16], dtype=np.int64)) == 1189480  # 195950 + 769400 + 224130
    # blend, t - d = -5: 40960 + 2048 - 20485 = 22523 -> floor(5.4988) = 5. Dividing the signed product alone and
    # truncating, 10 + trunc((2048 - 20485) / 4096) = 10 - 4, gives 6: the shift must be of the signed sum.
    i64 = np.int64
    assert O.blend(i64(5), i64(10), 4097) == 5
    assert 10 + int((2048 - 4097 * 5) / 4096) == 6
    assert O.blend(i64(0), i64(100), 8192) == 0  # 409600 + 2048 - 819200 < 0: clamped at 0
    assert O.blend(i64(1), i64(100), 8192) == 0  # floor(-97.5) = -98, clamped
    assert O.blend(i64(T), i64(0), 8192) == T  # 2 T: clamped at T
    assert O.blend(i64(T - 1), i64(0), 4097) == T  # T - 1 + floor((T - 1) / 4096 + 0.5) > T
    assert O.blend(i64(1000), i64(0), 2048) == 500 and O.blend(i64(1001), i64(0), 2048) == 501  # 500.5 + 0.5 -> 501
    # M of a 2x2 image of grey pixels (grey(v, v, v) = v): (65536 + 0 + 131072 + 3 + 2) // 4 = 196613 // 4
    img = np.array([[[65536] * 3, [0] * 3], [[131072] * 3, [3] * 3]], dtype=np.int64)
    assert list(O.grey(img).ravel()) == [65536, 0, 131072, 3] and O.mean_grey(img) == 49153
    # contrast 0.5 alone (order CBS, the others at one): t' = (4096 * 49153 + 2048 + 2048 (t - 49153)) >> 12
    got = O.jitter_image(img, O.ORDERS.index("CBS"), 4096, 2048, 4096)
    assert list(got[..., 0].ravel()) == [57345, 24577, 90113, 24578]  # t = 3: 2048 * 49157 / 4096 = 24578.5, floor
    # saturation 2 on one pixel: grey(30, 10, 20) = (587850 + 384700 + 149420 + 32768) >> 16 = 17; 17 + 2 (t - 17)
    px = np.array([[[30, 10, 20]]], dtype=np.int64)
    assert list(O.jitter_image(px, 0, 4096, 4096, 8192).ravel()) == [43, 3, 23]
    # brightness 1.5 clamps the bright pixel only
    px = np.array([[[T, 2, 0]]], dtype=np.int64)
    assert list(O.jitter_image(px, 0, 6144, 4096, 4096).ravel()) == [T, 3, 0]
    # a one-pixel image is its own mean: contrast moves it by its own grey only
    px = np.array([[[100, 100, 100]]], dtype=np.int64)
    assert list(O.jitter_image(px, 2, 4096, 1234, 4096).ravel()) == [100, 100, 100]


def test_order_matters_and_follows_the_table():
    assert O.ORDERS == ("BCS", "BSC", "CBS", "CSB", "SBC", "SCB")
    rng = np.random.default_rng(3)
    t = rng.integers(0, T + 1, size=(5, 4, 3)).astype(np.int64)
    outs = [O.jitter_image(t, o, 5000, 3000, 6000) for o in range(6)]
    assert all(np.any(outs[i] != outs[j]) for i in range(6) for j in range(i))
    # BCS by hand: brightness, then contrast about the brightened image's mean, then saturation
    b = O.blend(t, np.int64(0), 5000)
    c = O.blend(b, np.int64(O.mean_grey(b)), 3000)
    assert np.array_equal(outs[0], O.blend(c, O.grey(c)[..., None], 6000))


def test_factor_one_returns_the_input_in_every_order():
    rng = np.random.default_rng(4)
    t = rng.integers(0, T + 1, size=(6, 7, 3)).astype(np.int64)
    t[0, 0], t[0, 1] = 0, T
    for order in range(6):
        assert np.array_equal(O.jitter_image(t, order, 4096, 4096, 4096), t)
    assert O.bounds(0, 0, 0) == (4096,) * 6
    assert O.bounds(0.4, 0.4, 0.4) == (2458, 5734) * 3 and O.bounds(2.0, (0.5, 1.5), 0) == (0, 12288, 2048, 6144, 4096, 4096)


# ------------------------------------------------------------------------------------ against float64
def rounding_bound(jitter):
    """See test_integer_definition_is_the_float_formula_up_to_rounding."""
    phi = [f / 4096 for f in jitter]
    a, c = max(p + abs(1 - p) for p in phi), max(abs(1 - p) for p in phi) + 0.5
    e = 0.0
    for _ in range(3):
        e = a * e + c
    return e


def _case_blends(size):
    """(blend t, draw) of the six samples of the GPU test's main comparison at one output size."""
    Hs, Ws, _ = J.STORE
    X, _ = K.u8(J.STORE)
    k = R.constants(Hs, Ws, K.MEAN[3], K.STD[3])
    jit = O.bounds(*J.FULL)
    for b, s in enumerate(J.SRC):
        box = R.random_box(b, Hs, Ws, k, J.SEED, J.COUNTER)
        yield (O.blend_taps(X[s], box, R.flips(b, J.SEED, J.COUNTER), *size), O.draw(b, jit, J.SEED, J.COUNTER))


def test_integer_definition_is_the_float_formula_up_to_rounding():
    """The integer transform against the same formulas in float64 with nothing rounded between the steps.

    The allowed difference is derived, not chosen. Let e bound |integer t - real t| (units of 2^-16 pixel)
    before an operation with real factor phi = f / 4096 (the same number on both sides: Q12 is exact in
    float64). The real result is phi t + (1 - phi) d. The integer one is that expression on the integer t and
    d, rounded by at most 1/2 (the + 2048 and the floor). The integer d differs from the real d by at most e +
    1: brightness has d = 0; the grey level is a convex combination of the pixel's channels (error <= e) and
    adds 1/2 by its own rounding; the mean of grey levels adds another 1/2. The clamps are 1-Lipschitz. So

        e' <= phi e + |1 - phi| (e + 1) + 1/2 = (phi + |1 - phi|) e + |1 - phi| + 1/2,    e_0 = 0

    (the blend itself is exact in both). Three operations with the worst factor of the range in use: for 0.4
    (phi up to 5734 / 4096) e_3 = 5.44. The difference measured on these cases is below 2."""
    jit = O.bounds(*J.FULL)
    bound = rounding_bound(jit)
    assert bound == pytest.approx(5.44, abs=0.01)
    assert rounding_bound((4096,) * 6) == 0.5 * 3  # factors of one: only the roundings, and those are exact here
    worst = 0.0
    for size in J.OUTPUTS:
        for t, d in _case_blends(size):
            diff = np.abs(O.jitter_image(t, *d) - O.jitter_image_float(t, *d)).max()
            worst = max(worst, float(diff))
    print("integer vs float64: worst %.3f units of 2^-16 pixel, bound %.3f" % (worst, bound))
    assert 0 < worst <= bound


# ------------------------------------------------------------------------------------ the cases' reach
def test_gpu_cases_reach_every_order_both_clamps_and_contrast_first_and_last():
    jit = O.bounds(*J.FULL)
    draws = [O.draw(n, jit, J.SEED, J.COUNTER) for n in range(len(J.SRC))]
    assert [d[0] for d in draws] == [5, 3, 0, 4, 1, 2]  # all six orders among keys 0..5
    names = [O.ORDERS[d[0]] for d in draws]
    assert any(n[0] == "C" for n in names) and any(n[2] == "C" for n in names)
    assert all(2458 <= f <= 5734 for d in draws for f in d[1:]) and len({d[1:] for d in draws}) == 6
    X, y = K.u8(J.STORE)
    k = R.constants(12, 12, K.MEAN[3], K.STD[3])
    for size in [(8, 8), (7, 5), (16, 16)]:
        trace = {}
        out, labels, got = O.batch(X, y, J.SRC, size, k, jit, seed=J.SEED, counter=J.COUNTER, trace=trace)
        assert got == draws and trace["lo"] and trace["hi"], (size, trace)
        assert trace["peak"] < 1 << 42  # every intermediate fits 64-bit integers with room
        assert np.array_equal(labels, y[J.SRC]) and out.dtype == np.float32
        plain, _, _ = R.batch(X, y, J.SRC, size, k, augment=True, seed=J.SEED, counter=J.COUNTER)
        assert all(np.any(out[b] != plain[b]) for b in range(len(J.SRC)))
    # shards: the second half's keys continue the first's
    assert [O.draw(n, jit, J.SEED, J.COUNTER) for n in range(6, 12)] == \
        O.batch(X, y, J.SRC, (8, 8), k, jit, base=6, seed=J.SEED, counter=J.COUNTER)[2]


def test_pinned_factors_equal_the_plain_oracle():
    X, y = K.u8(J.STORE)
    k = R.constants(12, 12, K.MEAN[3], K.STD[3])
    for size in J.OUTPUTS:
        a, la, _ = O.batch(X, y, J.SRC + [99], size, k, (4096,) * 6, base=3, seed=J.SEED, counter=J.COUNTER)
        b, lb, _ = R.batch(X, y, J.SRC + [99], size, k, augment=True, base=3, seed=J.SEED, counter=J.COUNTER)
        assert np.array_equal(a, b) and np.array_equal(la, lb) and la[-1] == -1 and not a[-1].any()


# ------------------------------------------------------------------------------------ host checks
ARGS = ("data", "labels", "n_data", "idx", "first", "X", "y", "B", "Hs", "Ws", "C", "Ho", "Wo", "augment", "a_lo", "a_hi",
        "ratio", "q_lo", "q_hi", "ch", "cw", "shift", "scale_c", "base", "seed", "counter", "fb_lo", "fb_hi", "fc_lo",
        "fc_hi", "fs_lo", "fs_hi", "work", "work_len")


def _jitter_args(**over):
    """A full argument list of lbt_batch_resized_crop_jitter with fake non-NULL pointers (never dereferenced:
    every case below is rejected on the host first)."""
    p = ctypes.c_void_p(0x1000)
    a = dict(data=p, labels=p, n_data=37, idx=None, first=0, X=p, y=p, B=5, Hs=12, Ws=10, C=3, Ho=8, Wo=8, augment=1,
             a_lo=10, a_hi=120, ratio=p, q_lo=49152, q_hi=87381, ch=11, cw=9, shift=p, scale_c=p, base=0, seed=1,
             counter=2, fb_lo=2458, fb_hi=5734, fc_lo=2458, fc_hi=5734, fs_lo=2458, fs_hi=5734, work=p, work_len=40)
    a.update(over)
    return [a[k] for k in ARGS] + [None]


# everything lbt_batch_resized_crop refuses (tests/test_resized_crop.py's list, but C = 32: C != 3 is this
# entry point's own), with augment on and with it off where the plain launch is what runs ...
PLAIN_CASES = [dict(data=None), dict(labels=None), dict(X=None), dict(y=None), dict(ratio=None), dict(shift=None),
               dict(scale_c=None), dict(B=0), dict(B=-1), dict(Hs=0), dict(Ws=0), dict(Ho=0), dict(Wo=-1),
               dict(n_data=0), dict(n_data=-5), dict(Hs=8193, a_hi=120), dict(Ws=8193), dict(Ho=8193), dict(Wo=8193),
               dict(a_lo=0), dict(a_lo=-1), dict(a_lo=50, a_hi=49), dict(a_hi=121),
               dict(q_lo=0), dict(q_lo=-1), dict(q_lo=87382), dict(q_hi=1 << 32),
               dict(ch=0), dict(ch=13), dict(cw=0), dict(cw=11),
               dict(base=-1), dict(base=(1 << 32) - 4), dict(base=1 << 40),
               dict(first=-1), dict(first=33), dict(first=1 << 40)]
# ... and its own: the channel count, the factor ranges, the scratch (8 rows of 5 samples: 40 strips of one row)
OWN_CASES = [dict(C=0), dict(C=-3), dict(C=1), dict(C=4), dict(C=32),
             dict(fb_lo=-1), dict(fb_lo=5735), dict(fb_hi=65537), dict(fc_lo=-1), dict(fc_lo=5735), dict(fc_hi=65537),
             dict(fs_lo=-1), dict(fs_lo=5735), dict(fs_hi=65537), dict(fs_lo=1 << 30, fs_hi=1 << 30),
             dict(work=None), dict(work_len=39), dict(work_len=0), dict(work_len=-1),
             dict(work=None, fc_lo=4096, fc_hi=4097), dict(work_len=39, fc_lo=4095, fc_hi=4096)]
_ids = lambda o: ",".join("%s=%s" % kv for kv in o.items())  # noqa: E731


@pytest.mark.parametrize("augment", [1, 0])
@pytest.mark.parametrize("over", PLAIN_CASES, ids=_ids)
def test_jitter_refuses_what_the_plain_launch_refuses(over, augment):
    assert _lib.load().lbt_batch_resized_crop_jitter(*_jitter_args(augment=augment, **over)) == 1001


@pytest.mark.parametrize("over", OWN_CASES, ids=_ids)
def test_jitter_host_checks_return_einval(over):
    assert _lib.load().lbt_batch_resized_crop_jitter(*_jitter_args(**over)) == 1001


def test_scratch_size_follows_the_strip_policy():
    work = _lib.load().lbt_batch_resized_crop_jitter_work
    for B, Ho in ((5, 8), (1, 1), (6, 16), (12, 97), (256, 224), (32, 224), (300, 10), (1100, 10), (1, 8192), (3, 48)):
        want = (1024 + B - 1) // B
        rows = min(4096, max(1, (Ho + want - 1) // want))
        assert work(B, Ho) == B * ((Ho + rows - 1) // rows), (B, Ho)
    assert work(12, 97) == 12 * 49 and work(256, 224) == 1024 and work(5, 8) == 40
    assert work(0, 8) == -1 and work(5, 0) == -1 and work(5, 8193) == -1 and work(-1, -1) == -1


# ------------------------------------------------------------------------------------ the dataset class
def test_dataset_color_jitter_arguments():
    X, y = K.u8((6, 8, 3), n=6)
    m, s = K.MEAN[3], K.STD[3]
    ds = ResizedCropDataset(X, y, m, s, 4, device="cpu")
    assert ds.jitter is None
    ds = ResizedCropDataset(X, y, m, s, 4, device="cpu", color_jitter=(0.4, 0.4, 0.4))
    assert ds.jitter == (2458, 5734) * 3 == O.bounds(0.4, 0.4, 0.4)
    assert (ds.fb_lo, ds.fb_hi, ds.fc_lo, ds.fc_hi, ds.fs_lo, ds.fs_hi) == ds.jitter
    ds = ResizedCropDataset(X, y, m, s, 4, device="cpu", color_jitter=(2.0, (0.5, 1.5), 0, 0))  # hue 0 is no hue
    assert ds.jitter == (0, 12288, 2048, 6144, 4096, 4096)
    ds = ResizedCropDataset(X, y, m, s, 4, device="cpu", color_jitter=(0.4, 0, 0.4, (0, 0)))
    assert ds.jitter == (2458, 5734, 4096, 4096, 2458, 5734) and ds._jitter_work(5) is None  # contrast off: no scratch
    for bad in ((0.4, 0.4, 0.4, 0.1), (0, 0, 0, (-0.1, 0.1)),  # hue is not built
                (-0.1, 0, 0), (0, -1, 0), (0, 0, -0.5), (float("nan"), 0, 0),  # negative
                ((1.5, 0.5), 0, 0), (0, (1.2, 0.8), 0), (0, 0, (1.0, 0.9)), ((-0.5, 1.0), 0, 0),  # min > max, min < 0
                (0, 0, 16.5), ((0.0, 17.0), 0, 0), (0.4, 0.4), (0.4,) * 5, ((0.5, 1.0, 1.5), 0, 0)):
        with pytest.raises(ValueError):
            ResizedCropDataset(X, y, m, s, 4, device="cpu", color_jitter=bad)
    X1, y1 = K.u8((6, 8, 1), n=6)
    assert ResizedCropDataset(X1, y1, K.MEAN[1], K.STD[1], 4, device="cpu").jitter is None
    with pytest.raises(ValueError):  # jitter needs three channels
        ResizedCropDataset(X1, y1, K.MEAN[1], K.STD[1], 4, device="cpu", color_jitter=(0.4, 0.4, 0.4))
    with pytest.raises(ValueError):  # no host fallback: the kernel is the only way to a batch
        import torch
        ResizedCropDataset(X, y, m, s, 4, device="cpu", color_jitter=(0.4, 0.4, 0.4)).batch(
            torch.empty(2, 4, 4, 3), torch.empty(2, dtype=torch.int32), augment=True)
