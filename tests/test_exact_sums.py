"""tests/exact_sums.py, the exact reference of the frame's fixed-point pixel sums, against hand-worked cases (CPU only)."""
import numpy as np

import exact_sums as X

U = 2.0 ** -26


def dump(rows, width=1, height=1):
    """a dump of (r, g, b) rows, spp = len(rows) // (width * height), draw counts 0"""
    a = np.zeros((len(rows), 4), np.float32)
    a[:, :3] = np.asarray(rows, np.float32)
    return a


def test_truncates_toward_zero_and_drops_non_finite_samples():
    rows = [(U * 2.75, -U * 2.75, -0.0), (1.0, -1.0, 0.5), (np.nan, 1.0, 1.0), (np.inf, 0.0, 0.0), (0.0, -np.inf, 0.0)]
    sums, clamped = X.frame_sums(dump(rows), 1, 1, 5)
    assert sums.tolist() == [[[2 + 2 ** 26, -2 - 2 ** 26, 2 ** 25]]]      # +-2.75 units -> +-2; -0 -> 0; three samples dropped
    assert clamped == 0
    img, _ = X.exact_image(dump(rows), 1, 1, 5)
    assert img.dtype == np.float32
    want = (np.float32(2 + 2 ** 26) * np.float32(U)) / np.float32(5)
    assert img[0, 0, 0] == want and img[0, 0, 1] == -want


def test_values_straddling_the_small_path_and_the_clamp():
    spp = 4
    c = X.accum_clamp_for(spp)                      # min(1e10, 1.3e11 / 4) = 1e10
    assert c == np.float32(1e10)
    assert X.accum_clamp_for(100) == np.float32(1.3e11) / np.float32(100)
    below = np.nextafter(np.float32(31.999), np.float32(0))
    rows = [(31.999, -31.999, 0.0),                 # the small path's last value
            (32.0, below, 0.0),                     # a component above 31.999: the 64-bit path, no clamp
            (1e10, -1e10, 3.0),                     # exactly the clamp: not counted
            (2e10, 0.5, -3e10)]                     # beyond it: clamped to +-1e10 and counted once
    sums, clamped = X.frame_sums(dump(rows), 1, 1, spp)
    fx = lambda v: int(np.trunc(np.float32(v) * np.float32(2 ** 26)))
    want = [fx(31.999) + fx(32.0) + fx(1e10) + fx(1e10),
            fx(-31.999) + fx(below) + fx(-1e10) + fx(0.5),
            0 + 0 + fx(3.0) + fx(-1e10)]
    assert sums[0, 0].tolist() == want
    assert clamped == 1


def test_clamp_follows_spp_and_budget():
    rows = [(5e9, 0.0, 0.0)] * 2 + [(0.0, 0.0, 0.0)] * 62       # 64 spp: clamp 1.3e11 / 64 = 2.03e9
    s, clamped = X.frame_sums(dump(rows), 1, 1, 64)
    c = X.accum_clamp_for(64)
    assert clamped == 2 and s[0, 0, 0] == 2 * int(np.trunc(c * np.float32(2 ** 26)))
    _, clamped = X.frame_sums(dump(rows), 1, 1, 64, budget=4)     # progressive: the budget's clamp (1e10)
    assert clamped == 0


def test_pixels_are_the_dumps_rows_in_raster_order():
    w, h, spp = 3, 2, 2
    rng = np.random.default_rng(5)
    a = dump(rng.uniform(-2, 2, (w * h * spp, 3)))
    sums, _ = X.frame_sums(a, w, h, spp)
    for y in range(h):
        for x in range(w):
            pix = y * w + x
            want = [int(np.trunc(a[pix * spp + s, k] * np.float32(2 ** 26))) for k in range(3) for s in range(spp)]
            assert sums[y, x].tolist() == [want[0] + want[1], want[2] + want[3], want[4] + want[5]]
