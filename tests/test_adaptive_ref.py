"""CPU checks of tests/adaptive_ref.py, the numpy restatement of the adaptive judge that tests/test_gpu_adaptive.py holds the library
to: edge tiles, zero variance, the gates, partitions, and agreement with vk_progress_stderr's formula."""
import numpy as np

import adaptive_ref as R


def moments(width, height, k, window, seed=0, sigma=0.1, const=None):
    """running sums and moments of k windows of `window` samples of N(0.5, sigma) per component (const: every sample that value)"""
    rng = np.random.default_rng(seed)
    run = np.zeros((height, width, 3), np.int64)
    m2 = np.zeros((height, width, 3))
    for _ in range(k):
        if const is None:
            s = rng.normal(0.5, sigma, (height, width, 3, window))
        else:
            s = np.full((height, width, 3, window), const)
        w = np.rint(s * R.ACCUM_SCALE).astype(np.int64).sum(-1)
        run += w
        m2 += (w.astype(np.float64) * (1.0 / R.ACCUM_SCALE)) ** 2 / window
    return run, m2


def test_zero_variance_converges_at_zero_tolerance():
    run, m2 = moments(16, 16, 4, 8, const=0.25)
    frozen = R.judge(run, m2, np.zeros((2, 2), np.uint32), 32, 4, 0.0, 0.0, 0, 2)
    assert frozen.all()
    _, v = R.variance(run, m2, 32, 4)
    assert (v <= 0.0).all()


def test_tolerance_decides():
    run, m2 = moments(16, 16, 8, 16, sigma=0.2)
    se = np.sqrt(np.maximum(R.variance(run, m2, 128, 8)[1], 0.0))
    assert not R.judge(run, m2, np.zeros((2, 2)), 128, 8, float(se.min()) * 0.5, 0.0, 0, 2).any()
    assert R.judge(run, m2, np.zeros((2, 2)), 128, 8, float(se.max()) * 1.01, 0.0, 0, 2).all()
    # relative: |mean| ~ 0.5
    assert R.judge(run, m2, np.zeros((2, 2)), 128, 8, 0.0, float(se.max()) * 2.2 / 0.4, 0, 2).all()


def test_edge_tiles_pixels_outside_the_image_do_not_block():
    width, height = 13, 11                                   # 2 x 2 tiles, three of them cut by the image's edge
    run, m2 = moments(width, height, 4, 8, const=0.5)
    frozen = R.judge(run, m2, np.zeros((2, 2)), 32, 4, 0.0, 0.0, 0, 2)
    assert frozen.shape == (2, 2) and frozen.all()
    assert (R.tile_pixels(width, height) == np.array([[64, 40], [24, 15]])).all()


def test_one_noisy_pixel_keeps_its_tile_active():
    run, m2 = moments(16, 16, 4, 8, const=0.5)
    noisy_run, noisy_m2 = moments(16, 16, 4, 8, sigma=0.3, seed=3)
    run[10, 3], m2[10, 3] = noisy_run[10, 3], noisy_m2[10, 3]     # pixel (3, 10): tile (0, 1) (row 1 = the upper one, y up)
    frozen = R.judge(run, m2, np.zeros((2, 2)), 32, 4, 1e-3, 0.0, 0, 2)
    assert frozen.tolist() == [[True, True], [False, True]]


def test_gates():
    run, m2 = moments(16, 16, 4, 8, const=0.5)
    z = np.zeros((2, 2))
    assert not R.judge(run, m2, z, 32, 4, 1.0, 0.0, 33, 2).any()           # min_samples
    assert R.judge(run, m2, z, 32, 4, 1.0, 0.0, 32, 2).all()
    assert not R.judge(run, m2, z, 32, 4, 1.0, 0.0, 0, 5).any()            # min_steps
    assert R.judge(run, m2, z, 32, 4, 1.0, 0.0, 0, 4).all()


def test_frozen_and_foreign_tiles_are_never_judged_again():
    run, m2 = moments(24, 16, 4, 8, const=0.5)
    tn = np.array([[0, 7, 0], [0, 0, 0]], np.uint32)
    frozen = R.judge(run, m2, tn, 32, 4, 1.0, 0.0, 0, 2)
    assert frozen.tolist() == [[True, False, True], [True, True, True]]
    part = R.partition_mask(24, 16, 1, 4)
    assert part.tolist() == [[False, True, False], [False, False, True]]
    frozen = R.judge(run, m2, np.zeros((2, 3)), 32, 4, 1.0, 0.0, 0, 2, rank=1, world=4)
    assert (frozen == part).all()


def test_stderr_matches_the_library_formula_per_tile():
    """vk_progress_stderr: sqrt((sum_j n_j m_j^2 - N m^2) / ((k - 1) N)) from the windows' own means, each tile at its own N and k"""
    rng = np.random.default_rng(7)
    h, w = 16, 16
    wins = [rng.normal(0.5, 0.2, (h, w, 3, 8)) for _ in range(5)]
    tn, tk = np.array([[24, 40], [40, 16]]), np.array([[3, 5], [5, 2]])
    run = np.zeros((h, w, 3), np.int64)
    m2 = np.zeros((h, w, 3))
    want = np.zeros((h, w, 3))
    for ty in range(2):
        for tx in range(2):
            sl = (slice(8 * ty, 8 * ty + 8), slice(8 * tx, 8 * tx + 8))
            ws = [np.rint(x[sl] * R.ACCUM_SCALE).astype(np.int64).sum(-1) for x in wins[:tk[ty, tx]]]
            run[sl] = sum(ws)
            m2[sl] = sum((x * (1.0 / R.ACCUM_SCALE)) ** 2 / 8 for x in ws)
            N, k = float(tn[ty, tx]), float(tk[ty, tx])
            m_j = np.stack([x / R.ACCUM_SCALE / 8 for x in ws])
            m = run[sl] / R.ACCUM_SCALE / N
            want[sl] = np.sqrt(np.maximum((8 * m_j ** 2).sum(0) - N * m ** 2, 0) / ((k - 1) * N))
    got = R.stderr(run, m2, tn, tk)
    assert np.allclose(got, want, rtol=1e-5, atol=1e-7)
    # and the judge agrees with the estimate: a tile freezes exactly when max stderr <= abs_tol
    for ty in range(2):
        for tx in range(2):
            sl = (slice(8 * ty, 8 * ty + 8), slice(8 * tx, 8 * tx + 8))
            se = float(got[sl].max())
            for tol, expect in ((se * 1.001, True), (se * 0.999, False)):
                tmap = np.full((2, 2), 99, np.uint32)
                tmap[ty, tx] = 0
                d = R.judge(run, m2, tmap, int(tn[ty, tx]), int(tk[ty, tx]), tol, 0.0, 0, 2)
                assert d[ty, tx] == expect, (ty, tx, tol)
