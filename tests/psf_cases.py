"""The shared case list of the point-spread tests: the smallest shapes at which each mechanism can go wrong.  TESTS ONLY.

  1x1 K3            N = 4 in both directions, one pixel
  5x3 K3            Px 8, Py 8 from 7 and 5
  17x9 K9           odd sizes, Px 32, Py 32 (17 exactly)
  61x7 K5           Px 128, Py 16: not square
  60x4 K5, 61x4 K5  W + K - 1 = 64 exactly and 65: the power-of-two edge
  4000x2, 2x4000 K3 a 4096 line along x and along y with almost no other work
  321x181 K63       Px 512, Py 256: several lines per workgroup, rows the row pass skips
"""
import numpy as np

from glare_ref import hdr_frame

f32 = np.float32

# name, W, H, K, strength, threshold, seed, special values sown in
CASES = [
    ("1x1", 1, 1, 3, 0.15, 0.0, 1, False),
    ("5x3", 5, 3, 3, 0.15, 0.0, 2, False),
    ("17x9", 17, 9, 9, 0.3, 0.0, 3, True),
    ("61x7", 61, 7, 5, 0.15, 0.0, 4, False),
    ("60x4", 60, 4, 5, 1.0, 0.0, 5, False),
    ("61x4", 61, 4, 5, 0.15, 0.0, 6, True),
    ("4000x2", 4000, 2, 3, 0.15, 0.0, 7, False),
    ("2x4000", 2, 4000, 3, 0.15, 0.0, 8, False),
    ("321x181", 321, 181, 63, 0.15, 0.0, 9, True),
    ("17x9-threshold", 17, 9, 9, 0.5, 1.5, 10, True),
    ("61x7-threshold", 61, 7, 5, 0.15, 0.25, 11, False),
    ("17x9-zero-strength", 17, 9, 9, 0.0, 0.0, 12, True),
]
# the subset the numpy restatement is run on where a test has both yardsticks
SUBSET = ["1x1", "5x3", "17x9", "61x4", "2x4000", "17x9-threshold"]


def kernel(K, seed):
    """a random (K, K, 3) kernel: peaked, a different one per channel, some taps exactly zero; not normalised"""
    rng = np.random.default_rng(1000 + seed)
    k = rng.uniform(0, 1, (K, K, 3)) ** 6
    k[rng.uniform(0, 1, (K, K, 3)) < 0.2] = 0.0
    r = (K - 1) // 2
    k[r, r] += 2.0
    return k.astype(f32)


def frame(W, H, seed, special):
    return hdr_frame(W, H, seed, special)


def case(name):
    for c in CASES:
        if c[0] == name:
            return c
    raise KeyError(name)


def inputs(name):
    """(I, kernel, strength, threshold) of a case"""
    _, W, H, K, strength, threshold, seed, special = case(name)
    return frame(W, H, seed, special), kernel(K, seed), strength, threshold
