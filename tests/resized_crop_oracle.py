"""numpy restatement of lbt_batch_resized_crop (include/lbt_dfxp.h): the ImageNet input transform --
RandomResizedCrop + RandomHorizontalFlip or a centre crop, bilinear resample, Normalize -- in integers.

The reference (data.py:58-93, torchvision's transforms) gives the distribution; its draws are not
reproducible, so the draws are pinned by Philox as oracle.aux.augment_draws pins preprocess_image's. Boxes
are computed in Python integers (math.isqrt is the floor of the root), the resample in int64 numpy, the
normalisation in float64 with one rounding to fp32."""
import math

import numpy as np

from oracle.aux import AUG_STREAM
from oracle.philox import philox4x32_10

F32 = np.float32
RRC_STREAM = 0x52524321  # "RRC!"
FALLBACK = 10  # the attempt index of a box that ten rejections left to the central crop


def constants(Hs, Ws, mean, std, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """What the host prepares once (ResizedCropDataset's attributes of the same names)."""
    a_lo = max(1, int(math.ceil(scale[0] * Hs * Ws)))
    a_hi = max(a_lo, int(math.floor(scale[1] * Hs * Ws)))
    k = (np.arange(256, dtype=np.float64) + 0.5) / 256
    table = np.rint(65536 * np.exp(np.log(ratio[0]) + k * (np.log(ratio[1]) - np.log(ratio[0])))).astype(np.uint32)
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    return dict(a_lo=a_lo, a_hi=a_hi, ratio_q16=table, q_lo=int(np.rint(65536 * ratio[0])),
                q_hi=int(np.rint(65536 * ratio[1])), shift=65536.0 * 255.0 * mean, scale_c=1.0 / (65536.0 * 255.0 * std))


def of_dataset(ds):
    """The same dict read from a ResizedCropDataset: kernel and oracle then read the same numbers."""
    return {k: getattr(ds, k) for k in ("a_lo", "a_hi", "ratio_q16", "q_lo", "q_hi", "shift", "scale_c")}


def _draw(n, stream, seed, counter):
    r = philox4x32_10(np.uint32(n), np.uint32(stream), np.uint32(counter & 0xFFFFFFFF),
                      np.uint32((counter >> 32) & 0xFFFFFFFF), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return [int(v) for v in r]


def random_box(n, Hs, Ws, k, seed, counter):
    """(top, left, h, w, attempt) of sample n: attempt 0..9 accepted, FALLBACK after ten rejections."""
    for t in range(10):
        r = _draw(n, RRC_STREAM + t, seed, counter)
        a = k["a_lo"] + r[0] % (k["a_hi"] - k["a_lo"] + 1)
        q = int(k["ratio_q16"][r[1] >> 24])
        if q == 0:
            continue
        w = (math.isqrt((4 * a * q) >> 16) + 1) >> 1
        h = (math.isqrt(((4 * a) << 16) // q) + 1) >> 1
        if 1 <= w <= Ws and 1 <= h <= Hs:
            return r[2] % (Hs - h + 1), r[3] % (Ws - w + 1), h, w, t
    h, w = Hs, Ws
    if Ws * 65536 < k["q_lo"] * Hs:
        h = max(1, min(Hs, (2 * Ws * 65536 + k["q_lo"]) // (2 * k["q_lo"])))
    elif Ws * 65536 > k["q_hi"] * Hs:
        w = max(1, min(Ws, (2 * Hs * k["q_hi"] + 65536) >> 17))
    return (Hs - h) // 2, (Ws - w) // 2, h, w, FALLBACK


def center_box(Hs, Ws, center):
    ch, cw = center
    return (Hs - ch) // 2, (Ws - cw) // 2, ch, cw, -1


def flips(n, seed, counter):
    return _draw(n, AUG_STREAM, seed, counter)[0] & 1


def taps(inn, out, frac="round"):
    """Per output index: lower tap, upper tap, the upper tap's weight in 1/256 (half-pixel centres)."""
    i = np.arange(out, dtype=np.int64)
    n = np.clip((2 * i + 1) * inn - out, 0, (inn - 1) * 2 * out)
    p0 = n // (2 * out)
    rem = n - p0 * 2 * out
    f = (rem * 256 + (out if frac == "round" else 0)) // (2 * out)
    return p0, np.minimum(p0 + 1, inn - 1), f


def resample(img, box, flip, Ho, Wo, k, frac="round", norm="f64"):
    """One uint8 image [Hs, Ws, C] -> fp32 [Ho, Wo, C]. frac="trunc" and norm="f32" are the cheaper
    formulations the tests show to differ (never what the kernel may compute)."""
    top, left, h, w = box[:4]
    y0, y1, fy = taps(h, Ho, frac)
    x0, x1, fx = taps(w, Wo, frac)
    if flip:
        x0, x1, fx = x0[::-1], x1[::-1], fx[::-1]
    p = img[top:top + h, left:left + w].astype(np.int64)
    fy, fx = fy[:, None, None], fx[None, :, None]
    t = ((256 - fy) * ((256 - fx) * p[y0][:, x0] + fx * p[y0][:, x1])
         + fy * ((256 - fx) * p[y1][:, x0] + fx * p[y1][:, x1]))
    assert t.min() >= 0 and t.max() <= 255 * 65536
    if norm == "f32":
        return (t.astype(F32) - k["shift"].astype(F32)) * k["scale_c"].astype(F32)
    return ((t.astype(np.float64) - k["shift"]) * k["scale_c"]).astype(F32)


def batch(X, y, src, size, k, *, augment=False, center=None, base=0, seed=0, counter=0):
    """The batch of source samples ``src`` (indices into X / y): (out fp32 [B, Ho, Wo, C], labels int32 [B],
    boxes [(top, left, h, w, attempt)]). Sample b draws as sample base + b; an index outside the dataset
    gives a zero image and label -1."""
    n, Hs, Ws, C = X.shape
    Ho, Wo = size
    out = np.zeros((len(src), Ho, Wo, C), dtype=F32)
    labels = np.full(len(src), -1, dtype=np.int32)
    boxes = []
    for b, s in enumerate(src):
        box = random_box(base + b, Hs, Ws, k, seed, counter) if augment else center_box(Hs, Ws, center)
        boxes.append(box)
        if 0 <= s < n:
            flip = augment and flips(base + b, seed, counter)
            out[b] = resample(X[s], box, flip, Ho, Wo, k)
            labels[b] = y[s]
    return out, labels, boxes
