"""numpy restatement of lbt_batch_ragged_crop and lbt_batch_ragged_crop_jitter (include/lbt_dfxp.h): the
transforms of tests/resized_crop_oracle.py and tests/color_jitter_oracle.py with every image at its own stored
size. Nothing is restated here: per sample, that sample's source image gives the constants, the box is drawn
inside its own H x W with the key base + b, and the resample, the jitter and the normalisation are those
modules' functions."""
import numpy as np

import color_jitter_oracle as O
import resized_crop_oracle as R


def center_of(H, W, center=None):
    """An image's validation box: the caller's (ch, cw), or the square of 7/8 of the short side (224 of 256)."""
    return tuple(center) if center is not None else ((7 * min(H, W) + 4) // 8,) * 2


def constants(images, mean, std, **opts):
    """R.constants per image (a list of dicts); q_lo, q_hi, ratio_q16, shift and scale_c are the same in all."""
    return [R.constants(im.shape[0], im.shape[1], mean, std, **opts) for im in images]


def table(images, center=None, **opts):
    """What the host puts into the lbt_image_geom records: [(offset, Hs, Ws, a_lo, a_hi, ch, cw)], the images
    packed densely in order."""
    rows, off = [], 0
    for im in images:
        H, W, C = im.shape
        k = R.constants(H, W, (0.0,) * C, (1.0,) * C, **opts)
        rows.append((off, H, W, k["a_lo"], k["a_hi"]) + center_of(H, W, center))
        off += H * W * C
    return rows


def batch(images, y, src, size, mean, std, *, augment=False, center=None, jitter=None, base=0, seed=0, counter=0,
          **opts):
    """The batch of source samples ``src`` (indices into images / y): (out fp32 [B, Ho, Wo, C], labels int32
    [B], boxes [(top, left, h, w, attempt)], None for a source outside the store). Sample b draws as sample
    base + b inside its own image; jitter: the six Q12 bounds, applied when augmenting. A source outside the
    store gives a zero image and label -1."""
    Ho, Wo = size
    C = images[0].shape[2]
    out = np.zeros((len(src), Ho, Wo, C), dtype=R.F32)
    labels = np.full(len(src), -1, dtype=np.int32)
    boxes = []
    for b, s in enumerate(src):
        if not 0 <= s < len(images):
            boxes.append(None)
            continue
        img = images[s]
        H, W = img.shape[:2]
        k = R.constants(H, W, mean, std, **opts)
        if augment:
            box = R.random_box(base + b, H, W, k, seed, counter)
        else:
            box = R.center_box(H, W, center_of(H, W, center))
        boxes.append(box)
        flip = augment and R.flips(base + b, seed, counter)
        if augment and jitter is not None:
            t = O.blend_taps(img, box, flip, Ho, Wo)
            out[b] = O.normalise(O.jitter_image(t, *O.draw(base + b, jitter, seed, counter)), k)
        else:
            out[b] = R.resample(img, box, flip, Ho, Wo, k)
        labels[b] = y[s]
    return out, labels, boxes
