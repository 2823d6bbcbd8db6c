"""Device-resident datasets: the input side of the epoch loop without the host.

The reference's ``load_data`` (``main.py:65-75``) turns the uint8 images into float64, subtracts the
per-pixel mean of the training set, divides by 128 and feeds fp32 batches from host memory. A
``DeviceDataset`` keeps the images on the device in their native uint8 (a quarter of the fp32 bytes) with
the float64 mean beside them, and ``batch()`` writes the batch a step reads with one kernel launch
(``lbt_batch_gather``): gather, that normalisation, and ``preprocess_image``'s flip + crop
(``trainer.py:24-28``) -- bit for bit what the host path feeds, with nothing crossing PCIe and nothing
synchronising per step. ``Trainer.train()`` / ``Trainer.evaluate()`` take one in place of the arrays.
"""
import numpy as np
import torch

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
