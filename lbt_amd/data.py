"""Device-resident datasets: the input side of the epoch loop without the host.

The reference's ``load_data`` (``main.py:65-75``) turns the uint8 images into float64, subtracts the
per-pixel mean of the training set, divides by 128 and feeds fp32 batches from host memory. A
``DeviceDataset`` keeps the images on the device in their native uint8 (a quarter of the fp32 bytes) with
the float64 mean beside them, and ``batch()`` writes the batch a step reads with one kernel launch
(``lbt_batch_gather``): gather, that normalisation, and ``preprocess_image``'s flip + crop
(``trainer.py:24-28``) -- bit for bit what the host path feeds, with nothing crossing PCIe and nothing
synchronising per step. ``Trainer.train()`` / ``Trainer.evaluate()`` take one in place of the arrays.

A ``ResizedCropDataset`` is the same for the reference's ImageNet pipeline (``data.py:58-93``): uint8 images
of one stored size on the device, and one ``lbt_batch_resized_crop`` launch per batch for
``RandomResizedCrop`` + ``RandomHorizontalFlip`` (or the validation centre crop), the bilinear resample and
``Normalize``; with ``color_jitter`` the training launch (``lbt_batch_resized_crop_jitter``) also applies
``ColorJitter``'s brightness, contrast and saturation. A ``RaggedCropDataset`` is that pipeline on images
of their own sizes, as the reference runs it: one byte array and a table of per-image geometry on the
device, and the same kernels reading each sample's record (``lbt_batch_ragged_crop`` / ``_jitter``). All
three classes give the Trainer's loops ``sample_shape``, ``train_batch`` and ``test_batch``.
"""
import numpy as np
import torch

from . import _lib
from .dfxp import ops


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


class DeviceDataset:
    """X [n, H, W, C] or [n, F] (F = one pixel of F channels: the PI_MNIST layout), uint8 or float32;
    y [n] integer labels (stored int32).

    uint8 X is stored as it is, with ``mean`` [H, W, C] float64: None computes this array's per-pixel
    mean (a training set); pass ``train.mean`` for the test set. float32 X is taken as already
    normalised and stored as it is; ``mean`` must then be None."""

    def __init__(self, X, y, mean=None, device=None):
        X, y = _host(X), _host(y)
        if X.dtype not in (np.uint8, np.float32):
            raise TypeError("DeviceDataset holds uint8 or float32 images, got %s" % X.dtype)
        if X.ndim not in (2, 4):
            raise ValueError("X must be [n, H, W, C] or [n, F], got shape %s" % (X.shape,))
        if not np.issubdtype(y.dtype, np.integer):
            raise TypeError("labels must be integers, got %s" % y.dtype)
        if y.ndim != 1 or len(y) != len(X):
            raise ValueError("X holds %d samples, y %s" % (len(X), y.shape))
        if len(X) == 0:
            raise ValueError("an empty dataset")
        self.shape = tuple(X.shape)
        if X.dtype == np.uint8:
            if mean is None:
                mean = X.mean(axis=0, dtype=np.float64)  # integer sums: exact in any order
            else:
                mean = np.array(_host(mean), dtype=np.float64)
                if mean.shape != X.shape[1:]:
                    raise ValueError("mean must have the sample's shape %s, got %s" % (X.shape[1:], mean.shape))
        elif mean is not None:
            raise ValueError("float32 data is stored as it is: mean must be None")
        self.mean = mean
        self.device = torch.device(device if device is not None else "cuda")
        n = len(X)
        hwc = X.shape[1:] if X.ndim == 4 else (1, 1, X.shape[1])
        self._data = torch.from_numpy(np.ascontiguousarray(X)).to(self.device).view((n,) + tuple(hwc))
        self._labels = torch.from_numpy(y.astype(np.int32)).to(self.device)
        self._mean = None if mean is None else torch.from_numpy(np.ascontiguousarray(mean)).to(self.device).view(hwc)

    def __len__(self):
        return self.shape[0]

    def host_float(self):
        """The fp32 array the host path is given: load_data's ((X - mean) / 128 in float64, one rounding to
        fp32), or the float data itself."""
        X = self._data.cpu().numpy().reshape(self.shape)
        if self.mean is None:
            return X
        return ((X.astype(np.float64) - self.mean) / 128).astype(np.float32)

    def upload_index(self, index, out=None):
        """A host index vector (a permutation, a sampler's draw) as the device int32 tensor ``batch(idx=...)``
        takes slices of. Its range is checked here, on the host, once for all its batches. ``out``: a device
        int32 tensor of the same length to overwrite instead of allocating."""
        index = torch.as_tensor(index)
        if index.is_cuda or index.dtype not in (torch.int32, torch.int64) or index.dim() != 1:
            raise ValueError("upload_index takes a one-dimensional host int32 / int64 index vector")
        if index.numel() and (int(index.min()) < 0 or int(index.max()) >= len(self)):
            raise IndexError("index out of range for a dataset of %d samples" % len(self))
        index = index.to(torch.int32)
        if out is None:
            return index.to(self.device)
        out.copy_(index)
        return out

    def batch(self, out_X, out_y, *, idx=None, first=0, pad=0, flip=False, base=0, seed=0, counter=0, check=True):
        """Write one batch into out_X [B, ...sample shape] fp32 / out_y [B] int32 on the current stream:
        sample b is source sample idx[b] (idx: a device int32 tensor of B indices) or first + b, normalised,
        then flipped / cropped with the draw of sample base + b of (seed, counter) -- Trainer.train() passes
        the context's seed and its global step. pad = 0, flip = False: a plain gather.
        check: verify idx's range (one min / max on the device, which synchronises); a slice of what
        ``upload_index`` returned was checked there and takes check=False."""
        B = out_X.shape[0]
        if tuple(out_X.shape[1:]) != self.shape[1:]:
            raise ValueError("out_X must be [B, %s], got %s" % (", ".join(map(str, self.shape[1:])), tuple(out_X.shape)))
        for t in (out_X, out_y) + (() if idx is None else (idx,)):
            if t.device != self._data.device:  # the kernel takes raw pointers
                raise ValueError("the dataset lives on %s, a batch tensor on %s" % (self._data.device, t.device))
        if idx is None:
            if first < 0 or first + B > len(self):
                raise IndexError("samples [%d, %d) of a dataset of %d" % (first, first + B, len(self)))
        elif check and idx.numel():
            lo, hi = torch.aminmax(idx)
            if int(lo) < 0 or int(hi) >= len(self):
                raise IndexError("idx out of range for a dataset of %d samples" % len(self))
        ox = out_X if out_X.dim() == 4 else out_X.view((B,) + tuple(self._data.shape[1:]))
        ops.batch_gather(self._data, self._mean, self._labels, ox, out_y, idx=idx, first=first, pad=pad, flip=flip,
                         base=base, seed=seed, counter=counter)
        return out_X, out_y

    # -- what the Trainer's epoch loops call, on either dataset class -------------------------
    @property
    def sample_shape(self):
        """Shape of one sample of a batch."""
        return tuple(self.shape[1:])

    def train_batch(self, out_X, out_y, *, idx, augment, base=0, seed=0, counter=0):
        """A training batch of the permutation slice idx (checked by ``upload_index``): preprocess_image's
        flip + pad-4 crop when augmenting, a plain gather otherwise."""
        return self.batch(out_X, out_y, idx=idx, pad=4 if augment else 0, flip=bool(augment), base=base, seed=seed,
                          counter=counter, check=False)

    def test_batch(self, out_X, out_y, *, first):
        """Test samples [first, first + B) as they are."""
        return self.batch(out_X, out_y, first=first)


def _jitter_range(v, name):
    """torchvision's ColorJitter argument -- a scalar v >= 0 for [max(0, 1 - v), 1 + v], or a (min, max) pair
    -- as the factor range (lo, hi) in Q12."""
    if np.ndim(v) == 0:
        v = float(v)
        if not v >= 0:
            raise ValueError("%s must be non-negative, got %s" % (name, v))
        lo, hi = max(0.0, 1.0 - v), 1.0 + v
    else:
        if len(v) != 2:
            raise ValueError("%s must be a scalar or a (min, max) pair, got %s" % (name, v))
        lo, hi = float(v[0]), float(v[1])
    if not 0 <= lo <= hi <= 16:
        raise ValueError("%s: the factor range must satisfy 0 <= min <= max <= 16, got (%s, %s)" % (name, lo, hi))
    return int(np.rint(4096 * lo)), int(np.rint(4096 * hi))


def _area_range(s0, s1, Hs, Ws):
    """RandomResizedCrop's area range (a_lo, a_hi), in pixels, inside a stored Hs x Ws -- ints, or int arrays
    for a table of images: the same float64 products either way."""
    a_lo = np.maximum(1, np.ceil(s0 * Hs * Ws).astype(np.int64))
    a_hi = np.maximum(a_lo, np.floor(s1 * Hs * Ws).astype(np.int64))
    return a_lo, a_hi


class _CropDataset:
    """What ResizedCropDataset and RaggedCropDataset share: everything about the transform that does not depend
    on an image's stored size -- the labels, the output size, ``Normalize``'s constants, the aspect-ratio
    table, the colour jitter and its scratch -- and the batch interface the Trainer's loops call. A subclass
    holds the store (``_data``) with its geometry and makes the launch (``_launch``)."""

    def _init_pipeline(self, y, n, C, mean, std, size, scale, ratio, color_jitter, device):
        y = _host(y)
        if not np.issubdtype(y.dtype, np.integer):
            raise TypeError("labels must be integers, got %s" % y.dtype)
        if y.ndim != 1 or len(y) != n:
            raise ValueError("the store holds %d samples, y %s" % (n, y.shape))
        if n == 0:
            raise ValueError("an empty dataset")
        Ho, Wo = (size, size) if isinstance(size, (int, np.integer)) else tuple(size)
        Ho, Wo = int(Ho), int(Wo)
        if min(C, Ho, Wo) < 1 or max(Ho, Wo) > 8192:
            raise ValueError("the output size must lie in [1, 8192] with a channel or more, got %dx%dx%d" % (Ho, Wo, C))
        mean, std = (np.array(_host(v), dtype=np.float64).reshape(-1) for v in (mean, std))
        if mean.shape != (C,) or std.shape != (C,):
            raise ValueError("mean and std must hold one value per channel (%d)" % C)
        if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std > 0)):
            raise ValueError("mean must be finite and std positive")
        s0, s1 = (float(v) for v in scale)
        r0, r1 = (float(v) for v in ratio)
        if not 0 < s0 <= s1 <= 1:
            raise ValueError("scale must satisfy 0 < scale[0] <= scale[1] <= 1, got %s" % (scale,))
        if not 0 < r0 <= r1:
            raise ValueError("ratio must satisfy 0 < ratio[0] <= ratio[1], got %s" % (ratio,))
        self.scale_range = (s0, s1)
        k = (np.arange(256, dtype=np.float64) + 0.5) / 256
        self.ratio_q16 = np.rint(65536 * np.exp(np.log(r0) + k * (np.log(r1) - np.log(r0))))
        self.q_lo, self.q_hi = int(np.rint(65536 * r0)), int(np.rint(65536 * r1))
        if self.q_lo < 1 or self.q_hi >= 1 << 32 or self.ratio_q16.min() < 1 or self.ratio_q16.max() >= 1 << 32:
            raise ValueError("ratio %s does not fit 16.16 fixed point" % (ratio,))
        self.ratio_q16 = self.ratio_q16.astype(np.uint32)
        self.shift = 65536.0 * 255.0 * mean
        self.scale_c = 1.0 / (65536.0 * 255.0 * std)
        self.jitter = None
        if color_jitter is not None:
            cj = tuple(color_jitter)
            if len(cj) not in (3, 4):
                raise ValueError("color_jitter must be (brightness, contrast, saturation), got %s" % (color_jitter,))
            if len(cj) == 4 and np.any(np.asarray(cj[3], dtype=np.float64) != 0):
                raise ValueError("hue jitter is not built: color_jitter's hue must be 0, got %s" % (cj[3],))
            if C != 3:
                raise ValueError("color_jitter needs a three-channel store, got %d channels" % C)
            (self.fb_lo, self.fb_hi), (self.fc_lo, self.fc_hi), (self.fs_lo, self.fs_hi) = (
                _jitter_range(v, name) for v, name in zip(cj, ("brightness", "contrast", "saturation")))
            self.jitter = (self.fb_lo, self.fb_hi, self.fc_lo, self.fc_hi, self.fs_lo, self.fs_hi)
        self._work = {}  # batch size -> the contrast pass's scratch, allocated at first use and kept
        self._n = n
        self.sample_shape = (Ho, Wo, C)
        self.mean, self.std = mean, std
        self.device = torch.device(device if device is not None else "cuda")
        self._labels = torch.from_numpy(y.astype(np.int32)).to(self.device)
        self._ratio = torch.from_numpy(self.ratio_q16.view(np.int32).copy()).to(self.device)  # the bit patterns
        self._shift = torch.from_numpy(self.shift).to(self.device)
        self._scale = torch.from_numpy(self.scale_c).to(self.device)

    def __len__(self):
        return self._n

    upload_index = DeviceDataset.upload_index

    def batch(self, out_X, out_y, *, idx=None, first=0, augment=False, base=0, seed=0, counter=0, check=True):
        """Write one batch into out_X [B, Ho, Wo, C] fp32 / out_y [B] int32 on the current stream: sample b is
        source sample idx[b] (a device int32 tensor of B indices) or first + b; augment: the random box and
        flip of sample base + b of (seed, counter) -- Trainer.train() passes the context's seed and its global
        step -- else the centre box. With ``color_jitter``, augment also draws that sample's jitter. check as in
        DeviceDataset.batch."""
        B = out_X.shape[0]
        if tuple(out_X.shape[1:]) != self.sample_shape:
            raise ValueError("out_X must be [B, %s], got %s" % (", ".join(map(str, self.sample_shape)), tuple(out_X.shape)))
        for t in (out_X, out_y) + (() if idx is None else (idx,)):
            if t.device != self._data.device:  # the kernel takes raw pointers
                raise ValueError("the dataset lives on %s, a batch tensor on %s" % (self._data.device, t.device))
        if idx is None:
            if first < 0 or first + B > len(self):
                raise IndexError("samples [%d, %d) of a dataset of %d" % (first, first + B, len(self)))
        elif check and idx.numel():
            lo, hi = torch.aminmax(idx)
            if int(lo) < 0 or int(hi) >= len(self):
                raise IndexError("idx out of range for a dataset of %d samples" % len(self))
        work = {"jitter": self.jitter, "work": self._jitter_work(B)} if augment and self.jitter is not None else None
        self._launch(out_X, out_y, work, idx=idx, first=first, augment=bool(augment), base=base, seed=seed,
                     counter=counter)
        return out_X, out_y

    def _jitter_work(self, B):
        """The contrast pass's scratch for batches of B (None with contrast off). One buffer per batch size,
        kept: launches on one stream reuse it in order, and a captured launch keeps its address."""
        if (self.fc_lo, self.fc_hi) == (4096, 4096):
            return None
        if B not in self._work:
            n = ops.batch_resized_crop_jitter_work(B, self.sample_shape[0])
            self._work[B] = torch.empty(n, dtype=torch.int64, device=self._data.device)
        return self._work[B]

    def train_batch(self, out_X, out_y, *, idx, augment, base=0, seed=0, counter=0):
        """A training batch of the permutation slice idx (checked by ``upload_index``): the random box and
        flip when augmenting, the validation transform otherwise."""
        return self.batch(out_X, out_y, idx=idx, augment=bool(augment), base=base, seed=seed, counter=counter,
                          check=False)

    def test_batch(self, out_X, out_y, *, first):
        """Test samples [first, first + B) through the validation transform."""
        return self.batch(out_X, out_y, first=first)


class ResizedCropDataset(_CropDataset):
    """The reference's ImageNet pipeline (``data.py:58-93``) from device memory: X [n, Hs, Ws, C] uint8 of
    one stored size (resized offline, e.g. to 256 x 256), y [n] integer labels; ``mean`` / ``std`` per
    channel in ``Normalize``'s units (of pixel / 255); ``size`` the output (Ho, Wo), or one int for both.

    ``batch(augment=True)`` is the training transform -- ``RandomResizedCrop(size, scale, ratio)``,
    ``RandomHorizontalFlip``, ``ToTensor``, ``Normalize`` -- and ``batch()`` the validation one: the central
    ``center`` = (ch, cw) box (default 7/8 of the store: 224 of 256, ``Resize(256)`` + ``CenterCrop(224)`` on a
    256 x 256 store) resampled to ``size``. One ``lbt_batch_resized_crop`` launch writes the fp32 batch; the
    transform is defined in integers (include/lbt_dfxp.h) on the constants prepared here once: ``a_lo``,
    ``a_hi`` (the box's area in pixels), ``ratio_q16`` (256 log-uniform aspect ratios, Q16), ``q_lo``,
    ``q_hi``, ``shift`` and ``scale_c`` (float64 per channel). Bilinear without antialiasing: keep the store
    near the output size. Images of their own sizes: ``RaggedCropDataset``.

    ``color_jitter`` = (brightness, contrast, saturation), each a scalar or a (min, max) pair with
    torchvision's meaning, adds ``ColorJitter`` to the training transform (three-channel stores; hue is not
    built: a fourth entry must be zero): ``batch(augment=True)`` then launches
    ``lbt_batch_resized_crop_jitter``, which draws each sample's order and factors from the Q12 ranges
    ``fb_lo`` .. ``fs_hi`` (``jitter`` holds all six) and works in integers on the resampled pixel. ``batch()``
    and ``test_batch`` never jitter. None: the launch is ``lbt_batch_resized_crop``."""

    def __init__(self, X, y, mean, std, size, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), center=None, device=None,
                 color_jitter=None):
        X = _host(X)
        if X.dtype != np.uint8:
            raise TypeError("ResizedCropDataset holds uint8 images, got %s" % X.dtype)
        if X.ndim != 4:
            raise ValueError("X must be [n, Hs, Ws, C], got shape %s" % (X.shape,))
        n, Hs, Ws, C = X.shape
        if n and (min(Hs, Ws) < 1 or max(Hs, Ws) > 8192):
            raise ValueError("the stored size must lie in [1, 8192], got %dx%d" % (Hs, Ws))
        self._init_pipeline(y, n, C, mean, std, size, scale, ratio, color_jitter, device)
        self.a_lo, self.a_hi = (int(v) for v in _area_range(*self.scale_range, Hs, Ws))
        if center is None:
            center = ((7 * Hs + 4) // 8, (7 * Ws + 4) // 8)
        self.center = (int(center[0]), int(center[1]))
        if not (1 <= self.center[0] <= Hs and 1 <= self.center[1] <= Ws):
            raise ValueError("the centre box %s does not fit the stored %dx%d" % (self.center, Hs, Ws))
        self.shape = tuple(X.shape)
        self._data = torch.from_numpy(np.ascontiguousarray(X)).to(self.device)

    def _launch(self, out_X, out_y, jitter, **kw):
        args = (self._data, self._labels, out_X, out_y, self._ratio, self._shift, self._scale)
        geo = dict(a_lo=self.a_lo, a_hi=self.a_hi, q_lo=self.q_lo, q_hi=self.q_hi, center=self.center)
        if jitter is not None:
            ops.batch_resized_crop_jitter(*args, **geo, **jitter, **kw)
        else:
            ops.batch_resized_crop(*args, **geo, **kw)


class RaggedCropDataset(_CropDataset):
    """ResizedCropDataset for images of differing stored size -- the reference's pipeline as it runs on real
    data (``data.py:58-93``): ``RandomResizedCrop`` draws its box inside each image's own H x W, and validation
    is ``Resize(256)`` of the short side, aspect ratio kept, + ``CenterCrop(224)``. ``images`` is a sequence of
    uint8 arrays [H_i, W_i, C] with one C (resized offline, e.g. to a short side of 256); every other argument
    keeps its meaning.

    The store is one byte array on the device, the images packed densely in order, beside a table of one
    ``lbt_image_geom`` record per image (``geom``, a numpy array of ``_lib.IMAGE_GEOM_DTYPE``): the image's
    byte offset, its H and W, its own area range ``a_lo`` / ``a_hi`` -- ResizedCropDataset's expressions on its
    own H x W -- and its validation box. ``center=None`` makes that box the square of side ``(7 * min(H, W) + 4)
    // 8``: 224 of a short side of 256, where the resample to ``size`` = 224 is the identity and a validation
    batch holds the image's central 224 x 224 pixels, normalised: the reference's validation transform exactly.
    ``center=(ch, cw)`` asks for those pixels of every image. The launches are ``lbt_batch_ragged_crop`` and,
    with ``color_jitter``, ``lbt_batch_ragged_crop_jitter``; the table is checked here
    (``lbt_image_geom_check``), once, because the launch cannot.

    The whole store lies in device memory: sized for sets that fit it (a short-side-256 ImageNet-1k does not fit
    one GPU's HBM)."""

    def __init__(self, images, y, mean, std, size, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), center=None, device=None,
                 color_jitter=None):
        images = [_host(im) for im in images]
        if not images:
            raise ValueError("an empty dataset")
        for i, im in enumerate(images):
            if im.dtype != np.uint8:
                raise TypeError("RaggedCropDataset holds uint8 images, image %d is %s" % (i, im.dtype))
            if im.ndim != 3:
                raise ValueError("image %d must be [H, W, C], got shape %s" % (i, im.shape))
            if im.shape[2] != images[0].shape[2]:
                raise ValueError("image %d has %d channels, image 0 has %d" % (i, im.shape[2], images[0].shape[2]))
        shapes = np.array([im.shape[:2] for im in images], dtype=np.int64)
        data = np.concatenate([im.reshape(-1) for im in images])
        self._build(data, shapes, images[0].shape[2], y, mean, std, size, scale, ratio, center, device, color_jitter)

    @classmethod
    def from_flat(cls, data, shapes, y, mean, std, size, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), center=None,
                  device=None, color_jitter=None):
        """The same from a store already packed: ``data`` a one-dimensional uint8 array holding the images
        densely in order, ``shapes`` [n, 2] their (H, W). The channel count is ``mean``'s length. The host
        array is uploaded as it is, never copied."""
        data, shapes = _host(data), _host(shapes)
        if data.dtype != np.uint8:
            raise TypeError("RaggedCropDataset holds uint8 images, got %s" % data.dtype)
        if data.ndim != 1:
            raise ValueError("data must be one-dimensional, got shape %s" % (data.shape,))
        if not np.issubdtype(shapes.dtype, np.integer) or shapes.ndim != 2 or shapes.shape[1] != 2:
            raise ValueError("shapes must be [n, 2] integers, got %s %s" % (shapes.dtype, shapes.shape))
        self = cls.__new__(cls)
        self._build(data, shapes.astype(np.int64), int(np.size(_host(mean))), y, mean, std, size, scale, ratio, center,
                    device, color_jitter)
        return self

    def _build(self, data, shapes, C, y, mean, std, size, scale, ratio, center, device, color_jitter):
        n = len(shapes)
        H, W = shapes[:, 0], shapes[:, 1]
        bad = np.flatnonzero((H < 1) | (H > 8192) | (W < 1) | (W > 8192))
        if bad.size:
            raise ValueError("image %d: the stored size must lie in [1, 8192], got %dx%d" % (bad[0], H[bad[0]], W[bad[0]]))
        nbytes = H * W * C
        if int(nbytes.sum()) != data.size:
            raise ValueError("the images hold %d bytes at %d channels, data %d" % (nbytes.sum(), C, data.size))
        self._init_pipeline(y, n, C, mean, std, size, scale, ratio, color_jitter, device)
        if center is None:
            ch = cw = (7 * np.minimum(H, W) + 4) // 8
        else:
            center = (int(center[0]), int(center[1]))
            ch, cw = np.full(n, center[0], dtype=np.int64), np.full(n, center[1], dtype=np.int64)
        self.center = center
        bad = np.flatnonzero((ch < 1) | (ch > H) | (cw < 1) | (cw > W))
        if bad.size:
            i = bad[0]
            raise ValueError("image %d: the centre box (%d, %d) does not fit the stored %dx%d" % (i, ch[i], cw[i], H[i], W[i]))
        geom = np.zeros(n, dtype=np.dtype(_lib.IMAGE_GEOM_DTYPE))
        geom["offset"] = np.cumsum(nbytes) - nbytes
        geom["Hs"], geom["Ws"], geom["ch"], geom["cw"] = H, W, ch, cw
        geom["a_lo"], geom["a_hi"] = _area_range(*self.scale_range, H, W)
        i = ops.image_geom_check(geom, C, data.size)
        if i != -1:
            raise ValueError("image %d: its record %s is not valid for a store of %d bytes" % (i, geom[max(i, 0)], data.size))
        self.geom, self.shapes, self.channels = geom, shapes, C
        self._data = torch.from_numpy(np.ascontiguousarray(data)).to(self.device)
        self._geom = torch.from_numpy(geom.view(np.uint8).reshape(n, geom.itemsize)).to(self.device)

    def _launch(self, out_X, out_y, jitter, **kw):
        args = (self._data, self._geom, self._labels, out_X, out_y, self._ratio, self._shift, self._scale)
        if jitter is not None:
            ops.batch_ragged_crop_jitter(*args, q_lo=self.q_lo, q_hi=self.q_hi, **jitter, **kw)
        else:
            ops.batch_ragged_crop(*args, q_lo=self.q_lo, q_hi=self.q_hi, **kw)


# what Trainer.train() / evaluate() take in place of arrays
DEVICE_DATASETS = (DeviceDataset, ResizedCropDataset, RaggedCropDataset)
