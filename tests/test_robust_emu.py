"""The robust film's resolve on the CPU: the kernel's own per-pixel code (vk_robust.h robust_resolve_pixel<K>, built with g++ into
tests/emu) against tests/robust_ref.py's numpy restatement of the header's definition — image and standard error, bit for bit, for every
K in 2..16 and all three modes over a few thousand random tables that hold empty buckets (j = 0, 1, 2, 3 .. K), exact ties in Y,
negative sums, all-equal means, unequal counts and sums near +-2^62; and the hand cases of the definition."""
import numpy as np
import pytest

import emu_robust_ffi as EMU
import robust_ref as R

f32 = np.float32
N = 3000


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


@pytest.mark.parametrize("K", range(2, 17))
def test_emulator_equals_the_restatement(K, emu):
    tab = R.random_tables(K, N, seed=1)
    j = (tab[:, :, 3] > 0).sum(axis=1)
    assert set(range(0, min(K, 3) + 1)) | {K} <= set(j.tolist())                      # j = 0, 1, 2, 3 and K all occur
    assert (tab[:, :, :3] < 0).any() and (np.abs(tab[:, :, :3]) > (1 << 61)).any()
    trimmed = 0
    for mode, trim in ((R.MEAN, 0), (R.TRIM, 1), (R.TRIM, 3), (R.TRIM, 0xFFFFFFFF), (R.GINI, 0)):
        want_rgb, want_se, _, t, _ = R.resolve(tab, mode, trim, details=True)
        got_rgb, got_se = EMU.resolve(tab, mode, trim)
        assert same_bits(got_rgb, want_rgb), (K, mode, trim, np.argwhere(got_rgb.view(np.uint32) != want_rgb.view(np.uint32))[:4])
        assert same_bits(got_se, want_se), (K, mode, trim, np.argwhere(got_se.view(np.uint32) != want_se.view(np.uint32))[:4])
        if mode == R.GINI:
            trimmed = int((t > 0).sum())
            assert (t[j < 4] == 0).all()
    assert trimmed > 0 or K < 4


def test_the_tables_hold_ties_and_unequal_counts():
    tab = R.random_tables(8, N, seed=1)
    _, _, j, _, _ = R.resolve(tab, R.MEAN, details=True)
    cnt = tab[:, :, 3]
    full = j == 8
    assert (cnt[full].min(axis=1) != cnt[full].max(axis=1)).any()
    m = tab[full][:, :, :3] / cnt[full][:, :, None]
    assert any(len(np.unique(p, axis=0)) < 8 for p in m)              # two buckets of one mean: a tie in Y
    assert any(len(np.unique(p, axis=0)) == 1 for p in m)             # all-equal means


def test_seven_ones_and_one_outlier(emu):
    """K = 8, seven buckets of mean exactly 1 and one of mean exactly 801: num = 5600, s = 808, G = 5600 / 6464, G * 8 / 2 = 3.47: t = 3
    = tmax; GINI keeps two buckets of mean 1 and gives exactly 1.0 where MEAN gives 101.0"""
    for where in range(8):
        means = np.ones(8)
        means[where] = 801.0
        for counts in (None, np.full(8, 5)):
            tab = R.table_of_means(means, counts)
            rgb, se, j, t, G = R.resolve(tab, R.GINI, details=True)
            assert j == 8 and t == 3 and G == f32(5600.0) / f32(6464.0)
            assert (rgb == f32(1.0)).all() and (se == 0).all()
            got, got_se = EMU.resolve(tab, R.GINI)
            assert (got == f32(1.0)).all() and (got_se == 0).all()
            mean, mean_se = EMU.resolve(tab, R.MEAN)
            assert (mean == f32(101.0)).all() and same_bits(mean, R.resolve(tab, R.MEAN)[0])
            assert same_bits(mean_se, R.resolve(tab, R.MEAN)[1]) and (mean_se > 0).all()
            # stderr of 7 x 1 and 1 x 801: sqrt(sum (m - 101)^2 / 56) = sqrt((7 * 100^2 + 700^2) / 56) = 100
            assert (mean_se == f32(100.0)).all()


def test_two_buckets_never_trim(emu):
    for K in (2, 5, 16):
        means = np.zeros(K)
        counts = np.zeros(K, np.int64)
        means[0], means[K - 1] = 1.0, 1.0e6
        counts[0] = counts[K - 1] = 3
        tab = R.table_of_means(means, counts)
        for mode, trim in ((R.GINI, 0), (R.TRIM, 1), (R.TRIM, 7)):
            rgb, se, j, t, _ = R.resolve(tab, mode, trim, details=True)
            assert j == 2 and t == 0
            got, got_se = EMU.resolve(tab, mode, trim)
            assert same_bits(got, rgb) and same_bits(got_se, se) and same_bits(got, EMU.resolve(tab, R.MEAN)[0])
            assert (got == f32(500000.5)).all() and (got_se > 0).all()


def test_a_huge_trim_is_trim_at_tmax(emu):
    for K in range(2, 17):
        tab = R.random_tables(K, 200, seed=5)
        j = (tab[:, :, 3] > 0).sum(axis=1)
        tmax = int(max(0, (K - 2) // 2))
        at_tmax, at_tmax_se = EMU.resolve(tab, R.TRIM, tmax)
        for trim in (tmax + 1, 1 << 31, 0xFFFFFFFF):
            got, got_se = EMU.resolve(tab, R.TRIM, trim)
            assert same_bits(got, at_tmax) and same_bits(got_se, at_tmax_se), (K, trim)
        _, _, _, t, _ = R.resolve(tab, R.TRIM, 0xFFFFFFFF, details=True)
        assert np.array_equal(t, np.where(j < 2, 0, (j - 2) // 2))


def test_empty_pixel_single_bucket_and_the_mean_ignores_trim(emu):
    tab = np.zeros((3, 4, 4), np.int64)
    tab[1, 2] = (3 << 26, 2 << 26, 1 << 26, 2)
    tab[2] = R.table_of_means([0.25, 0.5, 0.75, 1.0])
    for mode in R.MODES:
        rgb, se = EMU.resolve(tab, mode, 1)
        assert (rgb[0] == 0).all() and (se[0] == 0).all()
        assert rgb[1].tolist() == [1.5, 1.0, 0.5] and (se[1] == 0).all()
    assert same_bits(EMU.resolve(tab, R.MEAN, 9)[0], EMU.resolve(tab, R.MEAN, 0)[0])
    assert same_bits(EMU.resolve(tab, R.GINI, 9)[0], EMU.resolve(tab, R.GINI, 0)[0])
    assert EMU.resolve(tab, R.TRIM, 1)[0][2].tolist() == [0.625] * 3 and EMU.resolve(tab, R.MEAN)[0][2].tolist() == [0.625] * 3


def test_negative_first_bucket_switches_gini_off(emu):
    """G's guard: with Y_1 < 0 (or a sum of Y that is not positive) GINI trims nothing, whatever the spread"""
    means = np.array([-0.5, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 5000.0])
    tab = R.table_of_means(means)
    rgb, se, j, t, G = R.resolve(tab, R.GINI, details=True)
    assert j == 8 and t == 0 and G == 0
    got, got_se = EMU.resolve(tab, R.GINI)
    assert same_bits(got, rgb) and same_bits(got_se, se) and same_bits(got, EMU.resolve(tab, R.MEAN)[0])
    means[0] = 0.5
    assert R.resolve(R.table_of_means(means), R.GINI, details=True)[3] == 3
