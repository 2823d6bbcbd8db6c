"""numpy restatement of lbt_batch_resized_crop_jitter (include/lbt_dfxp.h): the resized crop of
tests/resized_crop_oracle.py with ColorJitter's brightness, contrast and saturation between the bilinear blend
and the normalisation, in integers (Python ints inside int64 numpy: every intermediate is below 2^42).

The blend is restated here because resized_crop_oracle.resample returns the normalised fp32; the boxes, flips,
taps and draws are that module's. ``batch_float`` is the same transform in float64 with no rounding between the
steps: what the integer definition approximates (tests/test_color_jitter.py bounds the difference)."""
import numpy as np

from resized_crop_oracle import F32, _draw, flips, random_box, taps

CJT_STREAM = 0x434A5421  # "CJT!"
T = 255 * 65536  # the largest blend value: a pixel in units of 2^-16
ONE = 4096  # Q12
ORDERS = ("BCS", "BSC", "CBS", "CSB", "SBC", "SCB")  # the permutations of (B, C, S), lexicographic
GREY = (19595, 38470, 7471)  # PIL's "L" weights; they sum to 65536


def q12_range(v):
    """A ColorJitter argument (a scalar v >= 0 or a (min, max) pair) as the factor range (lo, hi) in Q12."""
    lo, hi = (max(0.0, 1.0 - v), 1.0 + v) if np.ndim(v) == 0 else (v[0], v[1])
    return int(np.rint(4096 * lo)), int(np.rint(4096 * hi))


def bounds(brightness, contrast, saturation):
    """The six Q12 bounds (fb_lo, fb_hi, fc_lo, fc_hi, fs_lo, fs_hi): ResizedCropDataset.jitter."""
    return q12_range(brightness) + q12_range(contrast) + q12_range(saturation)


def draw(n, jitter, seed, counter):
    """(order index, f_B, f_C, f_S) of sample n."""
    r = _draw(n, CJT_STREAM, seed, counter)
    f = [jitter[2 * i] + r[1 + i] % (jitter[2 * i + 1] - jitter[2 * i] + 1) for i in range(3)]
    return r[0] % 6, f[0], f[1], f[2]


def blend_taps(img, box, flip, Ho, Wo):
    """One uint8 image [Hs, Ws, C] -> the bilinear blend t, int64 [Ho, Wo, C] in [0, T]
    (resized_crop_oracle.resample before its normalisation)."""
    top, left, h, w = box[:4]
    y0, y1, fy = taps(h, Ho)
    x0, x1, fx = taps(w, Wo)
    if flip:
        x0, x1, fx = x0[::-1], x1[::-1], fx[::-1]
    p = img[top:top + h, left:left + w].astype(np.int64)
    fy, fx = fy[:, None, None], fx[None, :, None]
    t = ((256 - fy) * ((256 - fx) * p[y0][:, x0] + fx * p[y0][:, x1])
         + fy * ((256 - fx) * p[y1][:, x0] + fx * p[y1][:, x1]))
    assert t.min() >= 0 and t.max() <= T
    return t


def grey(t):
    """int64 [..., 3] -> [...]: (19595 R + 38470 G + 7471 B + 32768) >> 16."""
    return (GREY[0] * t[..., 0] + GREY[1] * t[..., 1] + GREY[2] * t[..., 2] + 32768) >> 16


def blend(t, d, f):
    """clamp(floor((4096 d + 2048 + f (t - d)) / 4096), 0, T); >> on int64 numpy is the arithmetic shift."""
    return np.clip((4096 * d + 2048 + f * (t - d)) >> 12, 0, T)


def mean_grey(t):
    """M of an image [Ho, Wo, 3]: (sum of grey + Ho Wo / 2) / (Ho Wo), in Python integers."""
    npx = t.shape[0] * t.shape[1]
    return (int(grey(t).sum()) + npx // 2) // npx


def jitter_image(t, order, fb, fc, fs, trace=None):
    """The three operations on the blend t [Ho, Wo, 3] in ORDERS[order]. trace: a dict that receives whether a
    clamp fired at 0 / at T ("lo", "hi")."""
    t = t.astype(np.int64)
    for op in ORDERS[order]:
        if op == "B":
            d, f = np.int64(0), fb
        elif op == "C":
            d, f = np.int64(mean_grey(t)), fc
        else:
            d, f = grey(t)[..., None], fs
        raw = (4096 * d + 2048 + f * (t - d)) >> 12
        if trace is not None:
            trace["lo"] = trace.get("lo", False) or bool((raw < 0).any())
            trace["hi"] = trace.get("hi", False) or bool((raw > T).any())
            trace["peak"] = max(trace.get("peak", 0), int(np.abs(4096 * d + 2048 + f * (t - d)).max()))
        t = np.clip(raw, 0, T)
    return t


def normalise(t, k):
    return ((t.astype(np.float64) - k["shift"]) * k["scale_c"]).astype(F32)


def batch(X, y, src, size, k, jitter, *, base=0, seed=0, counter=0, trace=None):
    """The training batch (augment) of source samples ``src`` with the jitter bounds ``jitter``: (out fp32 [B,
    Ho, Wo, 3], labels int32 [B], draws [(order, f_B, f_C, f_S)]). Sample b draws as sample base + b; an index
    outside the dataset gives a zero image and label -1."""
    n, Hs, Ws, C = X.shape
    assert C == 3
    Ho, Wo = size
    out = np.zeros((len(src), Ho, Wo, C), dtype=F32)
    labels = np.full(len(src), -1, dtype=np.int32)
    draws = []
    for b, s in enumerate(src):
        d = draw(base + b, jitter, seed, counter)
        draws.append(d)
        if 0 <= s < n:
            box = random_box(base + b, Hs, Ws, k, seed, counter)
            t = blend_taps(X[s], box, flips(base + b, seed, counter), Ho, Wo)
            out[b] = normalise(jitter_image(t, *d, trace=trace), k)
            labels[b] = y[s]
    return out, labels, draws


# ---------------------------------------------------------------- float64, nothing rounded between the steps
def jitter_image_float(t, order, fb, fc, fs):
    """The same formulas on float64 with real factors f / 4096, a real grey level and a real mean; only the
    clamps to [0, T] remain."""
    t = t.astype(np.float64)
    w = np.array(GREY, dtype=np.float64) / 65536
    for op in ORDERS[order]:
        if op == "B":
            d, f = 0.0, fb / 4096
        elif op == "C":
            d, f = (t * w).sum(axis=-1).mean(), fc / 4096
        else:
            d, f = (t * w).sum(axis=-1)[..., None], fs / 4096
        t = np.clip(d + f * (t - d), 0.0, float(T))
    return t
