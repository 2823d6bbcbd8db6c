"""The non-square geometry list of ``test_conv_geometry.py``, the kernel families it is run on, the
dispatch each (family, row) pair must take, and a direct loop-nest restatement of ``tf.nn.conv2d`` and
its two gradients (the independent check of the oracle on this list).

No GPU and no torch conv in here: importable by the CPU tests.
"""
import numpy as np

from lbt_amd._lib import OUT_F32, OUT_I8, OUT_I16, OUT_U8OFF

N = 2  # batch of every case

# id -> (H, W, KH, KW, SH, SW, padding)
ROWS = {
    "a": (6, 10, 3, 3, 1, 1, "SAME"),    # H vs W; the 3x3 fast paths (halo, wgrad3, stem row tiles)
    "b": (9, 5, 1, 3, 1, 1, "SAME"),     # KH vs KW; PT = 0 with PL = 1
    "c": (5, 9, 3, 1, 1, 1, "SAME"),     # the transpose of b
    "d": (7, 10, 3, 3, 2, 1, "SAME"),    # SH vs SW; two parity classes
    "e": (10, 7, 3, 3, 1, 2, "SAME"),    # the transpose of d
    "f": (8, 9, 3, 3, 2, 2, "VALID"),    # input row 7 unread: a class with taps and out-of-range sources
    "g": (9, 8, 2, 2, 2, 2, "SAME"),     # even kernel, pads (0, 1, 0, 0)
    "h": (7, 11, 3, 3, 3, 3, "SAME"),    # stride 3: nine classes, pads (1, 1, 0, 1)
    "i": (8, 6, 1, 1, 3, 2, "SAME"),     # unread rows and columns, five empty classes, wgrad1's pixel map
    "j": (8, 8, 4, 2, 2, 2, "SAME"),     # nk = 8 at Cin 64 (split-K 2), pads (1, 1, 0, 0)
    "k": (2, 3, 3, 5, 1, 1, "SAME"),     # kernel larger than the image; nk = 15 (split-K 3)
    "l": (6, 7, 3, 3, 1, 1, (2, 0)),     # explicit padding, Ho = 8 > H
    "m": (6, 7, 5, 3, 1, 2, "VALID"),    # everything differs at once
    "n": (9, 9, 3, 3, 4, 4, "VALID"),    # stride > kernel: rows and columns 3, 7, 8 unread
    # beyond the issue's fourteen: the table above has PT != PB on row g alone, and the discrimination
    # check asks for two such rows. 3x3 / 2 on an even height is the ResNets' own transition geometry.
    "o": (8, 5, 3, 3, 2, 2, "SAME"),     # pads (0, 1, 1, 1)
}
ROW_IDS = sorted(ROWS)
UNIT_STRIDE = [r for r in ROW_IDS if ROWS[r][4:6] == (1, 1)]

# resolved (Ho, Wo, pt, pb, pl, pr) and the input rows / columns no output window reads
GEOMETRY = {
    "a": (6, 10, 1, 1, 1, 1), "b": (9, 5, 0, 0, 1, 1), "c": (5, 9, 1, 1, 0, 0), "d": (4, 10, 1, 1, 1, 1),
    "e": (10, 4, 1, 1, 1, 1), "f": (3, 4, 0, 0, 0, 0), "g": (5, 4, 0, 1, 0, 0), "h": (3, 4, 1, 1, 0, 1),
    "i": (3, 3, 0, 0, 0, 0), "j": (4, 4, 1, 1, 0, 0), "k": (2, 3, 1, 1, 2, 2), "l": (8, 5, 2, 2, 0, 0),
    "m": (2, 3, 0, 0, 0, 0), "n": (2, 2, 0, 0, 0, 0), "o": (4, 3, 0, 1, 1, 1),
}
UNREAD = {  # rows, columns (every other row of the table reads all of its input)
    "f": ([7], []),
    "i": ([1, 2, 4, 5, 7], [1, 3, 5]),
    "n": ([3, 7, 8], [3, 7, 8]),
}


def geometry(row):
    """(Ho, Wo, pt, pb, pl, pr) from first principles (TF's SAME / VALID, or symmetric explicit pads)."""
    H, W, KH, KW, SH, SW, pad = ROWS[row]

    def axis(n, k, s, p):
        if pad == "VALID":
            return (n - k) // s + 1, 0, 0
        if pad == "SAME":
            out = (n + s - 1) // s
            total = max((out - 1) * s + k - n, 0)
            return out, total // 2, total - total // 2
        return (n + 2 * p - k) // s + 1, p, p

    ph, pw = pad if isinstance(pad, tuple) else (0, 0)
    Ho, pt, pb = axis(H, KH, SH, ph)
    Wo, pl, pr = axis(W, KW, SW, pw)
    return Ho, Wo, pt, pb, pl, pr


def unread(row):
    """([rows], [columns]) of the input that no output window of `row` reads."""
    H, W, KH, KW, SH, SW, _ = ROWS[row]
    Ho, Wo, pt, _, pl, _ = geometry(row)
    rows = {oh * SH + kh - pt for oh in range(Ho) for kh in range(KH)}
    cols = {ow * SW + kw - pl for ow in range(Wo) for kw in range(KW)}
    return [r for r in range(H) if r not in rows], [c for c in range(W) if c not in cols]


# ------------------------------------------------------------------------------ the loop nests
def conv_loops(x, w, g, row):
    """tf.nn.conv2d(x, w) on NHWC x HWIO integer codes, and with the output gradient g its
    conv2d_backprop_input and conv2d_backprop_filter: one loop nest over (n, oh, ow, kh, kw), the
    (ci, co) contraction in int64 numpy. Returns (y, dx, dw), int64."""
    H, W, KH, KW, SH, SW, _ = ROWS[row]
    Ho, Wo, pt, _, pl, _ = geometry(row)
    n_, _, _, Cin = x.shape
    Cout = w.shape[3]
    x, w, g = x.astype(np.int64), w.astype(np.int64), g.astype(np.int64)
    y = np.zeros((n_, Ho, Wo, Cout), np.int64)
    dx = np.zeros((n_, H, W, Cin), np.int64)
    dw = np.zeros((KH, KW, Cin, Cout), np.int64)
    for n in range(n_):
        for oh in range(Ho):
            for ow in range(Wo):
                for kh in range(KH):
                    ih = oh * SH + kh - pt
                    if not 0 <= ih < H:
                        continue
                    for kw in range(KW):
                        iw = ow * SW + kw - pl
                        if not 0 <= iw < W:
                            continue
                        y[n, oh, ow] += x[n, ih, iw] @ w[kh, kw]
                        dx[n, ih, iw] += w[kh, kw] @ g[n, oh, ow]
                        dw[kh, kw] += np.outer(x[n, ih, iw], g[n, oh, ow])
    return y, dx, dw


# ------------------------------------------------------------------------------ the kernel families
# name -> (bits, grad_bits, weight_bits, Cin, Cout, nonneg, bias): the smallest channel counts that
# select each kernel family
FAMILIES = {
    "mfma_u8": (8, None, None, 16, 32, True, False),        # register MFMA: offset codes, column sums, a_fill
    "mfma_s": (7, None, None, 32, 16, False, False),        # the same with signed codes
    "mfma_w4": (8, None, 4, 16, 16, True, False),           # the i8w4 entries
    "stem": (8, None, None, 3, 16, False, False),           # stem.hip where K <= 32, else stem_wide.hip
    "stem_64": (8, None, None, 3, 64, False, False),        # the same at stem.hip's widest Cout
    "stem_wide": (8, None, None, 3, 128, False, False),     # stem_wide.hip fwd and wgrad (row tiles: Cin <= 4)
    "igemm8_64_192": (8, None, None, 64, 192, False, False),   # int16 X codes (a_kind 2), 8-bit dgrad
    "igemm8_192_64": (8, None, None, 192, 64, True, False),    # offset codes (a_kind 1), the storing wgrad
    "igemm16_64_64": (8, 16, None, 64, 64, True, False),       # dgrad16, lbt_conv_wgrad_igemm_store
    "igemm16_128_128": (8, 16, None, 128, 128, True, False),   # ... with wgrad1 on row i
    "generic8": (8, None, None, 6, 10, False, True),        # conv_generic.hip int8 gradient codes
    "generic16": (8, 16, None, 6, 10, False, True),         # ... int16 gradient codes
    "fp32_12": (12, None, None, 5, 12, False, True),        # fp32.hip, exact
    "fp32_20": (20, None, None, 5, 12, False, True),        # fp32.hip, 1 ulp
}
FAMILY_IDS = sorted(FAMILIES)
IGEMM_FAMILIES = [f for f in FAMILY_IDS if f.startswith("igemm")]


def _path(fmode, x_kind, mfma=False, x_mfma=False, igemm_f=False, igemm_d=False, igemm_w=False, w4=False):
    return dict(fmode=fmode, x_kind=x_kind, mfma=mfma, x_mfma=x_mfma, igemm_f=igemm_f, igemm_d=igemm_d,
                igemm_w=igemm_w, w4=w4)


# The layer attributes that select a family's kernels (they depend on channels and widths only).
PATHS = {
    "mfma_u8": _path(False, OUT_U8OFF, mfma=True, x_mfma=True),
    "mfma_s": _path(False, OUT_I8, mfma=True, x_mfma=True),
    "mfma_w4": _path(False, OUT_U8OFF, mfma=True, x_mfma=True, w4=True),
    "stem": _path(False, OUT_I16),
    "stem_64": _path(False, OUT_I16),
    "stem_wide": _path(False, OUT_I16),
    "igemm8_64_192": _path(False, OUT_I16, igemm_f=True, igemm_d=True),
    "igemm8_192_64": _path(False, OUT_U8OFF, igemm_f=True, igemm_d=True, igemm_w=True),
    "igemm16_64_64": _path(False, OUT_U8OFF, igemm_f=True, igemm_d=True, igemm_w=True),
    "igemm16_128_128": _path(False, OUT_U8OFF, igemm_f=True, igemm_d=True, igemm_w=True),
    "generic8": _path(False, OUT_I16),
    "generic16": _path(False, OUT_I16),
    "fp32_12": _path(True, OUT_F32),
    "fp32_20": _path(True, OUT_F32),
}

# Per (family, row): which of the shape-dependent predicates hold. Everything not listed is False / 0.
# These are the contract's fallbacks written down:
#   stem.hip takes only K = KH*KW*Cin <= 32 and Cout in (16, 32, 64) -- rows k and m (K = 45) of the
#   3 -> 16 and 3 -> 64 families fall to stem_wide.hip, and so does every row at 3 -> 128 (its row-tile
#   form: Cin <= 4);
#   stem_wide.hip takes K <= 480 with exact fp32 sums (K <= 512 at these widths) and Cout % 16 == 0, so it
#   also takes the signed-code 64 -> 192 family on the windows of at most 4 taps (rows b, c, g, i: its
#   gather form), ahead of the implicit GEMM; the other rows of that family run the igemm forward with
#   int16 codes (a_kind 2);
#   wgrad3 takes only row a (3x3 / 1 / pad 1, 64 | Cin and Cout), wgrad1 only row i (1x1, 16-bit G, 128 |
#   Cin and Cout); both are consulted only by the layers with igemm_w.
STEM_ROWS = {"stem": set("abcdefghijlno"), "stem_64": set("abcdefghijlno")}
STEM_WIDE_ROWS = {"stem": set("km"), "stem_64": set("km"), "stem_wide": set(ROW_IDS), "igemm8_64_192": set("bcgi")}
WGRAD3_ROWS = {f: set("a") for f in ("igemm8_64_192", "igemm8_192_64", "igemm16_64_64", "igemm16_128_128")}
WGRAD1_WCI = {"igemm16_128_128": {"i": 2}}


def shape_path(family, row):
    """dict(stem, stem_wide, wgrad3, wgrad1) pinned for this pair."""
    return dict(stem=row in STEM_ROWS.get(family, ()), stem_wide=row in STEM_WIDE_ROWS.get(family, ()),
                wgrad3=row in WGRAD3_ROWS.get(family, ()), wgrad1=WGRAD1_WCI.get(family, {}).get(row, 0))


def fwd_on_igemm(family, row):
    """The forward of this pair is an implicit GEMM (so a forced 256-row kernel takes it)."""
    return PATHS[family]["igemm_f"] and not shape_path(family, row)["stem_wide"]
