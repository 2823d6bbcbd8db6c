"""The ragged image store without a GPU: the reach of the GPU test's cases (from the oracle's attempt index), the
ragged oracle against the uniform ones, the table RaggedCropDataset builds, lbt_image_geom_check, the record's
layout, the host checks of lbt_batch_ragged_crop / _jitter and the constructor's refusals."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import color_jitter_oracle as O
import ragged_crop_cases as G
import ragged_crop_oracle as RG
import resized_crop_cases as K
import resized_crop_oracle as R
from lbt_amd import _lib
from lbt_amd.data import DEVICE_DATASETS, RaggedCropDataset, ResizedCropDataset
from lbt_amd.dfxp import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------ the cases' reach
def _paths(opts):
    """The box paths the GPU test's batch takes under one option set, over both bases."""
    seen, flips = set(), set()
    for base in G.BASES:
        for b, s in enumerate(G.IDX):
            Hs, Ws = G.shape_of(s)
            k = R.constants(Hs, Ws, G.MEAN, G.STD, **opts)
            top, left, h, w, t = R.random_box(base + b, Hs, Ws, k, G.SEED, G.COUNTER)
            assert 1 <= h <= Hs and 1 <= w <= Ws and 0 <= top <= Hs - h and 0 <= left <= Ws - w
            flips.add(R.flips(base + b, G.SEED, G.COUNTER))
            if t == 0:
                seen.add("first")
            elif t < R.FALLBACK:
                seen.add("later")
            elif Ws * 65536 > k["q_hi"] * Hs:
                assert h == Hs and w < Ws and left == (Ws - w) // 2
                seen.add("columns cut")
            elif Ws * 65536 < k["q_lo"] * Hs:
                assert w == Ws and h < Hs and top == (Hs - h) // 2
                seen.add("rows cut")
            else:
                assert (top, left, h, w) == (0, 0, Hs, Ws)
                seen.add("whole")
    return seen, flips


def test_gpu_batch_reaches_every_path_of_the_box():
    assert G.BASES == (0, 3) and len(G.IDX) == 10 and max(G.IDX) == G.N_DATA - 1 and min(G.IDX) == 0
    assert len(set(G.IDX)) < len(G.IDX)  # a repeat
    assert {G.shape_of(s) for s in G.IDX} == set(G.SHAPES)  # every stored size is read
    seen, flips = _paths(G.OPTION_SETS[0])
    assert seen == {"first", "later", "columns cut", "rows cut", "whole"} and flips == {0, 1}
    seen, _ = _paths(G.OPTION_SETS[1])
    assert {"first", "later", "columns cut", "rows cut"} <= seen


def test_store_puts_images_at_odd_offsets():
    images, _ = G.store()
    rows = RG.table(images)
    assert [r[0] for r in rows[:4]] == [0, 432, 435, 813] and any(r[0] % 2 for r in rows)
    assert [(r[1], r[2]) for r in rows] == [G.shape_of(s) for s in range(G.N_DATA)]


# ------------------------------------------------------------------------------------ the oracle
def test_ragged_oracle_on_equal_images_is_the_uniform_oracle():
    X, y = K.u8((9, 14, 3))
    images = list(X)
    src = G.IDX + [99, -1]
    for opts in G.OPTION_SETS:
        k = R.constants(9, 14, G.MEAN, G.STD, **opts)
        for size in [(8, 8), (7, 5)]:
            for base in G.BASES:
                kw = dict(base=base, seed=G.SEED, counter=G.COUNTER)
                for augment in (True, False):
                    a, la, ba = RG.batch(images, y, src, size, G.MEAN, G.STD, augment=augment, center=(8, 12), **kw, **opts)
                    b, lb, bb = R.batch(X, y, src, size, k, augment=augment, center=(8, 12), **kw)
                    assert np.array_equal(a, b) and np.array_equal(la, lb) and ba[:-2] == bb[:-2]
                    assert la[-1] == la[-2] == -1 and not a[-2:].any()
                jit = O.bounds(0.4, 0.4, 0.4)
                a, la, _ = RG.batch(images, y, src, size, G.MEAN, G.STD, augment=True, jitter=jit, **kw, **opts)
                b, lb, _ = O.batch(X, y, src, size, k, jit, **kw)
                assert np.array_equal(a, b) and np.array_equal(la, lb)
    # the default centre box of a uniform store of squares is ResizedCropDataset's
    assert RG.center_of(256, 341) == (224, 224) and RG.center_of(12, 12) == (11, 11) and RG.center_of(5, 9, (2, 3)) == (2, 3)


def test_boxes_are_drawn_inside_each_image():
    """Two images of another size under the same key: other boxes. The key is the position, not the source."""
    images, y = G.store()
    _, _, boxes = RG.batch(images, y, [3, 4, 3], (8, 8), G.MEAN, G.STD, augment=True, seed=G.SEED, counter=G.COUNTER)
    assert boxes[0][2] <= 4 and boxes[1][3] <= 4 and boxes[0] != boxes[2]  # (4, 40), (40, 4); keys 0 and 2
    _, _, again = RG.batch(images, y, [3], (8, 8), G.MEAN, G.STD, augment=True, base=2, seed=G.SEED, counter=G.COUNTER)
    assert again[0] == boxes[2]


# ------------------------------------------------------------------------------------ the table
def test_dataset_table_is_the_oracles():
    images, y = G.store()
    for opts in G.OPTION_SETS:
        for center in (None, (1, 1)):
            ds = RaggedCropDataset(images, y, G.MEAN, G.STD, (7, 5), center=center, device="cpu", **opts)
            assert isinstance(ds, DEVICE_DATASETS) and len(ds) == G.N_DATA and ds.sample_shape == (7, 5, 3)
            assert ds.geom.dtype.itemsize == 32 and ds.geom.shape == (G.N_DATA,)
            assert [tuple(int(v) for v in r) for r in ds.geom] == RG.table(images, center, **opts)
            sizes = np.array([im.size for im in images])
            assert np.array_equal(ds.geom["offset"], np.cumsum(sizes) - sizes)
            for s, im in enumerate(images):
                k = R.constants(im.shape[0], im.shape[1], G.MEAN, G.STD, **opts)
                assert (ds.geom["a_lo"][s], ds.geom["a_hi"][s]) == (k["a_lo"], k["a_hi"])
            k = R.constants(1, 1, G.MEAN, G.STD, **opts)
            assert (ds.q_lo, ds.q_hi) == (k["q_lo"], k["q_hi"]) and np.array_equal(ds.ratio_q16, k["ratio_q16"])
            assert np.array_equal(ds.shift, k["shift"]) and np.array_equal(ds.scale_c, k["scale_c"])
            assert np.array_equal(ds._data.numpy(), np.concatenate([im.reshape(-1) for im in images]))
            assert ds._geom.dtype == torch.uint8 and tuple(ds._geom.shape) == (G.N_DATA, 32)
            assert ds._geom.numpy().tobytes() == ds.geom.tobytes() and ds._labels.dtype == torch.int32
    big = [np.zeros((256, 341, 3), np.uint8), np.zeros((500, 256, 3), np.uint8)]
    ds = RaggedCropDataset(big, [0, 1], G.MEAN, G.STD, 224, device="cpu")
    assert [(int(r["ch"]), int(r["cw"])) for r in ds.geom] == [(224, 224), (224, 224)]
    k = R.constants(256, 341, G.MEAN, G.STD)
    assert (ds.geom["a_lo"][0], ds.geom["a_hi"][0]) == (k["a_lo"], k["a_hi"]) == (6984, 87296)


def test_from_flat_is_the_same_dataset():
    images, y = G.store()
    a = RaggedCropDataset(images, y, G.MEAN, G.STD, 8, device="cpu", color_jitter=(0.4, 0.4, 0.4))
    flat = np.concatenate([im.reshape(-1) for im in images])
    shapes = np.array([im.shape[:2] for im in images])
    b = RaggedCropDataset.from_flat(flat, shapes, y, G.MEAN, G.STD, 8, device="cpu", color_jitter=(0.4, 0.4, 0.4))
    assert isinstance(b, RaggedCropDataset) and np.array_equal(a.geom, b.geom) and torch.equal(a._data, b._data)
    assert torch.equal(a._labels, b._labels) and a.jitter == b.jitter == O.bounds(0.4, 0.4, 0.4)
    assert b._data.numpy().ctypes.data == flat.ctypes.data  # uploaded as it is: no host copy
    for kw in (dict(data=flat[:-1]), dict(data=flat.astype(np.int8)), dict(data=flat.reshape(1, -1)),
               dict(shapes=shapes[:-1]), dict(shapes=shapes.astype(np.float32)), dict(shapes=shapes.reshape(-1)),
               dict(mean=K.MEAN[1], std=K.STD[1])):
        args = dict(data=flat, shapes=shapes, y=y, mean=G.MEAN, std=G.STD, size=8)
        args.update(kw)
        with pytest.raises((ValueError, TypeError)):
            RaggedCropDataset.from_flat(device="cpu", **args)


# ------------------------------------------------------------------------------------ lbt_image_geom_check
def _table(n=5):
    images, _ = G.store(n=n)
    t = np.array(RG.table(images), dtype=np.dtype(_lib.IMAGE_GEOM_DTYPE))
    return t, sum(im.size for im in images)


BAD_RECORDS = [dict(offset=-1), dict(offset=1 << 40), dict(Hs=0), dict(Hs=-4), dict(Hs=8193, a_hi=1), dict(Ws=0),
               dict(Ws=8193, a_hi=1), dict(a_lo=0), dict(a_lo=-1), dict(a_lo=3, a_hi=2), dict(ch=0), dict(cw=0), dict(ch=-1)]


@pytest.mark.parametrize("where", [0, 2, 4])
@pytest.mark.parametrize("over", BAD_RECORDS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_geom_check_names_the_first_bad_record(over, where):
    t, nbytes = _table()
    assert ops.image_geom_check(t, 3, nbytes) == -1
    for k, v in over.items():
        t[k][where] = v
    assert ops.image_geom_check(t, 3, nbytes) == where
    t["a_lo"][4] = 0  # a later bad record does not change the answer
    assert ops.image_geom_check(t, 3, nbytes) == where


def test_geom_check_bounds_are_exact():
    t, nbytes = _table()
    sizes = t["Hs"].astype(np.int64) * t["Ws"] * 3
    for s in range(len(t)):  # a store that ends with image s holds it and refuses the next
        assert ops.image_geom_check(t, 3, int(t["offset"][s] + sizes[s])) == (s + 1 if s + 1 < len(t) else -1)
    assert ops.image_geom_check(t, 3, nbytes - 1) == len(t) - 1
    for field, limit in (("a_hi", "px"), ("ch", "Hs"), ("cw", "Ws")):
        for s in (0, 3):
            u = t.copy()
            top = int(u["Hs"][s]) * int(u["Ws"][s]) if limit == "px" else int(u[limit][s])
            u[field][s] = top
            if field == "a_hi":
                u["a_lo"][s] = top
            assert ops.image_geom_check(u, 3, nbytes) == -1
            u[field][s] = top + 1
            assert ops.image_geom_check(u, 3, nbytes) == s
    one = np.zeros(1, dtype=t.dtype)
    one[0] = (0, 8192, 8192, 1, 1, 1, 1)
    assert ops.image_geom_check(one, 31, 1 << 40) == -1  # 31 * 2^26 < 2^31
    assert ops.image_geom_check(one, 32, 1 << 40) == 0  # Hs*Ws*C = 2^31
    assert ops.image_geom_check(one, 1, (1 << 26) - 1) == 0 and ops.image_geom_check(one, 1, 1 << 26) == -1


def test_geom_check_accepts_overlap_and_repeats_and_any_alignment():
    t, nbytes = _table()
    u = t[[0, 0, 2, 2, 4]].copy()  # an image listed twice
    assert ops.image_geom_check(u, 3, nbytes) == -1
    u["offset"] = [0, 1, 3, 5, 7]  # overlapping, odd offsets
    assert ops.image_geom_check(u, 3, nbytes) == -1


def test_geom_check_refuses_no_table_and_bad_scalars():
    t, nbytes = _table()
    check = _lib.load().lbt_image_geom_check
    p = t.ctypes.data_as(ctypes.c_void_p)
    assert check(p, 5, 3, nbytes) == -1
    assert check(None, 5, 3, nbytes) == -2 and check(p, 0, 3, nbytes) == -2 and check(p, -1, 3, nbytes) == -2
    assert check(p, 5, 0, nbytes) == -2 and check(p, 5, -3, nbytes) == -2
    assert check(p, 5, 3, 0) == -2 and check(p, 5, 3, -8) == -2
    assert ops.image_geom_check(t[:0], 3, nbytes) == -2


def test_record_layout_matches_c():
    py = _lib.ImageGeom
    assert ctypes.sizeof(py) == 32 == np.dtype(_lib.IMAGE_GEOM_DTYPE).itemsize
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lbt_dfxp.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(lbt_image_geom));']
    for f, _ in py._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(lbt_image_geom, %s));' % (f, f))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write("\n".join(lines))
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe], text=True).splitlines())
    assert int(out["size"]) == 32
    fields = np.dtype(_lib.IMAGE_GEOM_DTYPE).fields
    assert [f for f, _ in py._fields_] == ["offset", "Hs", "Ws", "a_lo", "a_hi", "ch", "cw"] == list(fields)
    for f, _ in py._fields_:
        assert int(out[f]) == getattr(py, f).offset == fields[f][1], f
    assert sum(ctypes.sizeof(t) for _, t in py._fields_) == 32  # no padding


# ------------------------------------------------------------------------------------ host checks
ARGS = ("data", "data_bytes", "geom", "labels", "n_data", "idx", "first", "X", "y", "B", "C", "Ho", "Wo", "augment", "ratio",
        "q_lo", "q_hi", "shift", "scale_c", "base", "seed", "counter")
JARGS = ARGS + ("fb_lo", "fb_hi", "fc_lo", "fc_hi", "fs_lo", "fs_hi", "work", "work_len")


def _args(names, **over):
    """A full argument list with fake non-NULL pointers (never dereferenced: every case below is rejected on
    the host first)."""
    p = ctypes.c_void_p(0x1000)
    a = dict(data=p, data_bytes=5000, geom=p, labels=p, n_data=37, idx=None, first=0, X=p, y=p, B=5, C=3, Ho=8, Wo=8,
             augment=1, ratio=p, q_lo=49152, q_hi=87381, shift=p, scale_c=p, base=0, seed=1, counter=2,
             fb_lo=2458, fb_hi=5734, fc_lo=2458, fc_hi=5734, fs_lo=2458, fs_hi=5734, work=p, work_len=40)
    a.update(over)
    return [a[k] for k in names] + [None]


# everything lbt_batch_resized_crop refuses that still has an argument (tests/test_resized_crop.py's list) ...
SHARED_CASES = [dict(data=None), dict(labels=None), dict(X=None), dict(y=None), dict(ratio=None), dict(shift=None),
                dict(scale_c=None), dict(B=0), dict(B=-1), dict(Ho=0), dict(Wo=-1), dict(n_data=0), dict(n_data=-5),
                dict(Ho=8193), dict(Wo=8193), dict(q_lo=0), dict(q_lo=-1), dict(q_lo=87382), dict(q_hi=1 << 32),
                dict(base=-1), dict(base=(1 << 32) - 4), dict(base=1 << 40),
                dict(first=-1), dict(first=33), dict(first=1 << 40),
                # ... and the table's own
                dict(geom=None), dict(data_bytes=0), dict(data_bytes=-1)]
PLAIN_ONLY = [dict(C=0), dict(C=-3), dict(Ho=8192, Wo=8192, C=32)]
# the jitter's own (tests/test_color_jitter.py's list): 8 rows of 5 samples are 40 strips of one row
JITTER_ONLY = [dict(C=0), dict(C=-3), dict(C=1), dict(C=4), dict(C=32),
               dict(fb_lo=-1), dict(fb_lo=5735), dict(fb_hi=65537), dict(fc_lo=-1), dict(fc_lo=5735), dict(fc_hi=65537),
               dict(fs_lo=-1), dict(fs_lo=5735), dict(fs_hi=65537), dict(fs_lo=1 << 30, fs_hi=1 << 30),
               dict(work=None), dict(work_len=39), dict(work_len=0), dict(work_len=-1),
               dict(work=None, fc_lo=4096, fc_hi=4097), dict(work_len=39, fc_lo=4095, fc_hi=4096)]
_ids = lambda o: ",".join("%s=%s" % kv for kv in o.items())  # noqa: E731


@pytest.mark.parametrize("over", SHARED_CASES + PLAIN_ONLY, ids=_ids)
def test_ragged_crop_host_checks_return_einval(over):
    assert _lib.load().lbt_batch_ragged_crop(*_args(ARGS, **over)) == 1001
    assert _lib.load().lbt_batch_ragged_crop(*_args(ARGS, augment=0, **over)) == 1001


@pytest.mark.parametrize("augment", [1, 0])
@pytest.mark.parametrize("over", SHARED_CASES, ids=_ids)
def test_ragged_jitter_refuses_what_the_plain_launch_refuses(over, augment):
    assert _lib.load().lbt_batch_ragged_crop_jitter(*_args(JARGS, augment=augment, **over)) == 1001


@pytest.mark.parametrize("over", JITTER_ONLY, ids=_ids)
def test_ragged_jitter_host_checks_return_einval(over):
    assert _lib.load().lbt_batch_ragged_crop_jitter(*_args(JARGS, **over)) == 1001


# ------------------------------------------------------------------------------------ the dataset class
def test_ragged_dataset_argument_checks():
    images, y = G.store(n=6)
    m, s = G.MEAN, G.STD

    def make(**kw):
        a = dict(images=images, y=y, mean=m, std=s, size=4)
        a.update(kw)
        return RaggedCropDataset(device="cpu", **a)

    for bad in (np.int16, np.float32):
        with pytest.raises(TypeError):
            make(images=images[:2] + [images[2].astype(bad)] + images[3:])
    with pytest.raises(TypeError):
        make(y=y.astype(np.float32))
    one = [np.zeros((6, 8, 1), np.uint8)] * 2
    for kw in (dict(images=[]), dict(y=y[:5]), dict(images=images[:3] + [images[3][:, :, 0]] + images[4:]),
               dict(mean=m[:2]), dict(std=(0.2, 0.0, 0.2)), dict(size=0), dict(size=(4, 8193)),
               dict(scale=(0.0, 1.0)), dict(scale=(0.5, 0.4)), dict(scale=(0.5, 1.5)),
               dict(ratio=(0.0, 1.0)), dict(ratio=(2.0, 1.0)), dict(ratio=(1.0, 70000.0)),
               dict(color_jitter=(0.4, 0.4, 0.4, 0.1)), dict(color_jitter=(-0.1, 0, 0)), dict(color_jitter=(0.4, 0.4)),
               dict(color_jitter=((1.5, 0.5), 0, 0)), dict(color_jitter=(0, 0, 16.5)),
               dict(images=one, y=y[:2], mean=K.MEAN[1], std=K.STD[1], color_jitter=(0.4, 0.4, 0.4))):
        with pytest.raises(ValueError):
            make(**kw)
    assert make(images=one, y=y[:2], mean=K.MEAN[1], std=K.STD[1]).jitter is None
    assert make(color_jitter=(2.0, (0.5, 1.5), 0, 0)).jitter == (0, 12288, 2048, 6144, 4096, 4096)
    assert make(color_jitter=(0.4, 0, 0.4))._jitter_work(5) is None  # contrast off: no scratch

    # the refusals that name the first offending image
    with pytest.raises(ValueError, match="image 1"):  # the 1x1 image
        make(center=(2, 2))
    with pytest.raises(ValueError, match="image 0"):
        make(center=(0, 1))
    four = [images[0], images[2], images[3], images[4]]  # (12, 12), (9, 14), (4, 40), (40, 4)
    with pytest.raises(ValueError, match="image 2"):  # (4, 40) has no five rows
        make(images=four, y=y[:4], center=(5, 1))
    with pytest.raises(ValueError, match="image 3"):  # (40, 4) has no five columns
        make(images=four, y=y[:4], center=(1, 5))
    assert make(images=four, y=y[:4], center=(4, 4)).center == (4, 4)
    wide = images[:2] + [np.zeros((1, 8193, 3), np.uint8)] + images[3:]
    with pytest.raises(ValueError, match="image 2"):
        make(images=wide)
    with pytest.raises(ValueError, match="image 2"):
        make(images=[im.transpose(1, 0, 2) for im in wide])
    with pytest.raises(ValueError, match="image 5"):
        make(images=images[:5] + [np.zeros((16, 16, 4), np.uint8)])
    with pytest.raises(ValueError, match="image 1"):  # an image without pixels
        make(images=[images[0], np.zeros((0, 5, 3), np.uint8)], y=y[:2])

    ds = make(images=[torch.from_numpy(im) for im in images], y=torch.from_numpy(y).long(), size=(4, 5))
    assert len(ds) == 6 and ds.sample_shape == (4, 5, 3) and ds.center is None and ds.channels == 3
    assert np.array_equal(ds.shapes, [G.shape_of(s) for s in range(6)])
    assert [int(v) for v in ds.geom["ch"]] == [11, 1, 8, 4, 4, 14] == [int(v) for v in ds.geom["cw"]]
    with pytest.raises(ValueError):  # no host fallback: the kernel is the only way to a batch
        ds.batch(torch.empty(2, 4, 5, 3), torch.empty(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        ds.batch(torch.empty(2, 5, 4, 3), torch.empty(2, dtype=torch.int32))
    with pytest.raises(IndexError):
        ds.upload_index(torch.tensor([0, 6]))
    assert ds.upload_index(torch.tensor([5, 0])).dtype == torch.int32
    for member in ("train_batch", "test_batch", "upload_index", "batch", "_jitter_work"):
        assert callable(getattr(ds, member)) and callable(getattr(ResizedCropDataset, member))
