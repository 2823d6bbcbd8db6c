"""The cases of tests/test_ragged_crop_gpu.py, shared with tests/test_ragged_crop.py, which checks on the CPU
(from the oracle's attempt index) that they reach every path of the box computation. SEED, COUNTER, BASES and
OUTPUTS are those of tests/resized_crop_cases.py."""
import numpy as np

import resized_crop_cases as K

N_DATA = 37
# the store cycles these: square, one pixel (every later image then starts at an odd byte offset), wide, very
# wide, very tall, square again, and a small odd one
SHAPES = [(12, 12), (1, 1), (9, 14), (4, 40), (40, 4), (16, 16), (7, 5)]
C = 3
IDX = [36, 0, 9, 9, 19, 3, 4, 2, 34, 13]  # a repeat, both ends, neighbours of different size
SEED, COUNTER, BASES, OUTPUTS = K.SEED, K.COUNTER, K.BASES, K.OUTPUTS
MEAN, STD = K.MEAN[3], K.STD[3]

# the area pinned to the whole image with ratios in [1/2, 2]: rejections and every fallback branch; and the defaults
OPTION_SETS = [dict(scale=(1.0, 1.0), ratio=(0.5, 2.0)), {}]
OPTION_IDS = ["whole-area", "defaults"]


def shape_of(s):
    return SHAPES[s % len(SHAPES)]


def store(n=N_DATA, seed=1, shapes=None):
    """(images, labels): n uint8 images [H, W, 3] cycling ``shapes`` (SHAPES), and int32 labels."""
    rng = np.random.default_rng(seed)
    shapes = SHAPES if shapes is None else shapes
    images = [rng.integers(0, 256, size=tuple(shapes[s % len(shapes)]) + (C,), dtype=np.uint8) for s in range(n)]
    return images, rng.integers(0, 10, size=n).astype(np.int32)
