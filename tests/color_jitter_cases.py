"""The cases of tests/test_color_jitter_gpu.py, shared with tests/test_color_jitter.py, which checks on the CPU
(from the oracle) that they reach what they claim to: all six orders, both clamps, contrast first and last.
The store, SEED and COUNTER are those of tests/resized_crop_cases.py."""
import resized_crop_cases as K

STORE = (12, 12, 3)
SRC = [36, 0, 7, 7, 19, 5]  # six samples at base 0: keys 0..5 draw the six orders; a repeat, both ends
OUTPUTS = K.OUTPUTS  # (8,8); (7,5): Wo*C = 15, pixels straddle quads; (16,16) upsamples; (1,1) is its own mean
FULL = (0.4, 0.4, 0.4)  # the reference's ColorJitter
# each operation alone, and contrast off (the launch without the statistics pass)
PARTIAL = [(0.4, 0, 0), (0, 0.4, 0), (0, 0, 0.4), (0.4, 0, 0.4)]
SEED, COUNTER = K.SEED, K.COUNTER
