"""The cases of tests/test_resized_crop_gpu.py, shared with tests/test_resized_crop.py, which checks on the
CPU (from the oracle's attempt index) that they reach every path of the box computation."""
import numpy as np

N_DATA = 37
IDX = [36, 0, 7, 7, 19]  # a repeat, both ends, unordered
SEED = 0x0123456789ABCDEF  # both key words in use
COUNTER = (1 << 32) + 77  # both counter words in use
BASES = (0, 3)
OUTPUTS = [(8, 8), (7, 5), (16, 16), (1, 1)]  # (16,16) upsamples; (7,5): Wo*C = 15 or 5, no whole quads

# (store, constructor options). (4,40,3) / (40,4,1) with scale >= 0.5: every attempt asks for more rows /
# columns than the store has (h >= 7 > 4), so the box is the fallback's wide / tall branch. (12,12,3) with
# the area and the ratio pinned is the whole image, accepted at once; with the area pinned and ratios in
# [1/2, 2] an attempt is accepted only for ratios in about (0.92, 1.085), so some samples are rejected ten
# times with the store's own ratio in range: the fallback's whole-image branch.
STORES = [((12, 12, 3), {}),
          ((9, 14, 3), {}),
          ((4, 40, 3), dict(scale=(0.5, 1.0))),
          ((40, 4, 1), dict(scale=(0.5, 1.0))),
          ((1, 1, 3), {}),
          ((12, 12, 3), dict(scale=(1.0, 1.0), ratio=(1.0, 1.0))),
          ((12, 12, 3), dict(scale=(1.0, 1.0), ratio=(0.5, 2.0)))]
STORE_IDS = ["12x12x3", "9x14x3", "4x40x3-wide", "40x4x1-tall", "1x1x3", "12x12x3-pinned", "12x12x3-whole"]

MEAN = {3: (0.485, 0.456, 0.406), 1: (0.449,)}  # no binary fractions
STD = {3: (0.229, 0.224, 0.225), 1: (0.226,)}


def u8(shape, n=N_DATA, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, size=(n,) + tuple(shape), dtype=np.uint8),
            rng.integers(0, 10, size=n).astype(np.int32))
