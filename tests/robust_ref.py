"""vk_robust_deposit and vk_robust_resolve restated in numpy float32 / int64 from the definition in include/vecchio_amd.h ("robust
film"), on top of tests/exact_sums.py and tests/film_ref.py.  The resolve is written pixel-vectorised and step by step in the header's
order: every f32 operation is one numpy operation on float32 arrays.  What tests/test_robust_emu.py and tests/test_gpu_robust.py share."""
import numpy as np

import exact_sums as E
import film_ref as F
from vecchio_amd import ffi
from vecchio_amd.scene import PATH_STATE_DTYPE

f32 = np.float32
MEAN, TRIM, GINI = ffi.VK_ROBUST_MEAN, ffi.VK_ROBUST_TRIM, ffi.VK_ROBUST_GINI
MODES = (MEAN, TRIM, GINI)
COUNTERS = ("deposited", "dropped", "clamped", "skipped")
INV_SCALE = f32(2.0 ** -26)


def deposit(states, status, width, height, spp, K, state=None):
    """vk_robust_deposit in numpy: (state (height, width, K, 4) int64 — added to where given —, dict of the four counters).  The
    film's rule (tests/film_ref.py deposit) with the bucket state.sample % K and a count that takes the dropped results too."""
    states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1)
    status = np.ascontiguousarray(status, np.uint32).reshape(-1)
    n_pixels = width * height
    state = np.zeros((height, width, K, 4), np.int64) if state is None else state.copy()
    flat = state.reshape(n_pixels * K, 4)
    ours = np.isin(status, F.DEPOSITING) & (states["pixel"] < n_pixels)
    acc = states["acc"].astype(f32)
    finite = np.isfinite(acc).all(axis=1)
    dep = ours & finite
    clampv = E.accum_clamp_for(spp)
    cell = states["pixel"].astype(np.int64) * K + (states["sample"].astype(np.int64) % K)
    big = np.abs(acc[dep]).max(axis=1) if dep.any() else np.zeros(0, f32)
    if dep.any():
        add = np.zeros((int(dep.sum()), 4), np.int64)
        add[:, :3] = E.to_fixed(acc[dep], clampv)
        np.add.at(flat, cell[dep], add)
    one = np.zeros((int(ours.sum()), 4), np.int64)
    one[:, 3] = 1
    np.add.at(flat, cell[ours], one)
    counters = dict(deposited=int(dep.sum()), dropped=int((ours & ~finite).sum()),
                    clamped=int(((big > E.ACCUM_SMALL) & (big > clampv)).sum()), skipped=int((~ours).sum()))
    return state, counters


def counters_of(info):
    return {k: int(getattr(info, k)) for k in COUNTERS}


def resolve(state, mode, trim=0, details=False):
    """vk_robust_resolve in numpy: state (..., K, 4) int64 -> (rgb (..., 3) float32, stderr (..., 3) float32); details: also (j, t, G)"""
    state = np.asarray(state, np.int64)
    K = state.shape[-2]
    shape = state.shape[:-2]
    tab = state.reshape(-1, K, 4)
    n = len(tab)
    cnt = tab[:, :, 3]
    ne = cnt > 0
    j = ne.sum(axis=1).astype(np.int64)
    with np.errstate(all="ignore"):
        # 2. the bucket means and their luminance
        nf = np.where(ne, cnt, 1).astype(f32)
        m = ((tab[:, :, :3].astype(f32) * INV_SCALE).astype(f32) / nf[:, :, None]).astype(f32)
        m = np.where(ne[:, :, None], m, f32(0.0)).astype(f32)
        Y = ((f32(0.2126) * m[:, :, 0] + f32(0.7152) * m[:, :, 1]).astype(f32) + f32(0.0722) * m[:, :, 2]).astype(f32)
        # 3. the order: non-empty buckets by Y, ties by index (a stable sort); the empty ones behind them
        key = np.where(ne, Y, f32(np.inf)).astype(f32)
        order = np.argsort(key, axis=1, kind="stable")
        empty_last = np.argsort(~np.take_along_axis(ne, order, axis=1), axis=1, kind="stable")      # (a non-empty Y may be +inf)
        order = np.take_along_axis(order, empty_last, axis=1)
        oY = np.take_along_axis(Y, order, axis=1)
        om = np.take_along_axis(m, order[:, :, None], axis=1)
        # 4. the trim
        tmax = np.where(j < 2, 0, (j - 2) // 2)
        G = np.zeros(n, f32)
        if mode == MEAN:
            t = np.zeros(n, np.int64)
        elif mode == TRIM:
            t = np.minimum(np.int64(trim), tmax)
        else:
            num, s = np.zeros(n, f32), np.zeros(n, f32)
            for i in range(K):
                live = i < j
                coef = (2 * (i + 1) - j - 1).astype(f32)
                num = np.where(live, (num + (coef * oY[:, i]).astype(f32)).astype(f32), num)
                s = np.where(live, (s + oY[:, i]).astype(f32), s)
            ok = (oY[:, 0] >= 0) & (s > 0) & (j > 0)
            G = np.where(ok, (num / (j.astype(f32) * s).astype(f32)).astype(f32), f32(0.0)).astype(f32)
            h = ((G * j.astype(f32)).astype(f32) * f32(0.5)).astype(f32)
            t = np.minimum(np.where(h >= 1, np.floor(np.where(h >= 1, h, f32(0.0))), 0).astype(np.int64), tmax)
        # 5. the kept set, in the order's positions
        pos = np.arange(K)[None, :]
        kept = (pos >= t[:, None]) & (pos < (j - t)[:, None])
        q = j - 2 * t
        # 6. the image: integer sums over the kept buckets (wrapping), one conversion, one division
        otab = np.take_along_axis(tab, order[:, :, None], axis=1)
        ks = np.where(kept[:, :, None], otab, 0).sum(axis=1, dtype=np.int64)
        den = np.where(j > 0, ks[:, 3], 1).astype(f32)
        rgb = ((ks[:, :3].astype(f32) * INV_SCALE).astype(f32) / den[:, None]).astype(f32)
        rgb = np.where((j > 0)[:, None], rgb, f32(0.0)).astype(f32)
        # 7. the standard error of the kept bucket means
        qf = np.where(q >= 2, q, 2).astype(f32)
        M = np.zeros((n, 3), f32)
        for i in range(K):
            M = np.where(kept[:, i, None], (M + om[:, i]).astype(f32), M)
        M = (M / qf[:, None]).astype(f32)
        e = np.zeros((n, 3), f32)
        for i in range(K):
            d = (om[:, i] - M).astype(f32)
            e = np.where(kept[:, i, None], (e + (d * d).astype(f32)).astype(f32), e)
        dd = np.where(q >= 2, q * (q - 1), 2).astype(f32)
        se = np.sqrt((e / dd[:, None]).astype(f32)).astype(f32)
        se = np.where((q >= 2)[:, None], se, f32(0.0)).astype(f32)
    rgb, se = rgb.reshape(shape + (3,)), se.reshape(shape + (3,))
    if details:
        return rgb, se, j.reshape(shape), t.reshape(shape), G.reshape(shape)
    return rgb, se


def table_of_means(means, counts=None):
    """one pixel's table (K, 4) whose bucket b holds counts[b] samples of colour means[b] (grey where a scalar), exactly"""
    means = np.asarray(means, np.float64)
    K = len(means)
    counts = np.ones(K, np.int64) if counts is None else np.asarray(counts, np.int64)
    tab = np.zeros((K, 4), np.int64)
    rgb = means if means.ndim == 2 else np.repeat(means[:, None], 3, axis=1)
    tab[:, :3] = np.round(rgb * 2.0 ** 26).astype(np.int64) * counts[:, None]
    tab[:, 3] = counts
    return tab


def random_tables(K, n, seed):
    """(n, K, 4) int64 tables that between them hold everything the resolve branches on: empty buckets (j from 0 to K), exact ties in
    Y, negative sums (G's guard), all-equal means, counts that differ between buckets, sums near +-2^62, outliers of every size, and
    negative or zero counts (empty)"""
    rng = np.random.default_rng(seed * 131 + K)
    tab = np.zeros((n, K, 4), np.int64)
    cnt = rng.integers(1, 40, (n, K))
    kind = rng.integers(0, 10, n)
    base = rng.random((n, 1, 3)) * 2.0
    noise = rng.random((n, K, 3)) * rng.choice([0.0, 0.01, 0.5, 2.0], (n, 1, 1))
    mean = base + noise
    spike = rng.random((n, K)) < rng.choice([0.0, 0.1, 0.3], (n, 1))
    mean = np.where(spike[:, :, None], mean * rng.choice([10.0, 1000.0, 1e6], (n, 1, 1)), mean)
    mean[kind == 1] = base[kind == 1]                                      # all-equal means
    cnt[kind == 1] = cnt[kind == 1][:, :1]
    mean[kind == 2] -= 1.5                                                 # negative sums
    mean[kind == 3] = np.round(mean[kind == 3] * 2.0) / 2.0                 # ties in Y, many
    cnt[kind == 3] = 1
    tab[:, :, :3] = np.round(mean * 2.0 ** 26).astype(np.int64) * cnt[:, :, None]
    tab[:, :, 3] = cnt
    huge = kind == 4                                                       # sums near +-2^62
    sign = rng.choice([-1, 1], (n, K, 3))
    near = (np.int64(1) << 62) - rng.integers(0, 1 << 40, (n, K, 3))
    tab[huge, :, :3] = (sign * near)[huge]
    positive = kind == 5                                                   # ... and of one sign, so that G is taken of them
    tab[positive, :, :3] = near[positive]
    # empty buckets: a share of the pixels loses a random subset, some all, some all but j = 1, 2, 3
    drop = rng.random((n, K)) < rng.choice([0.0, 0.0, 0.3, 0.7, 1.0], (n, 1))
    for want, rows in ((1, kind == 6), (2, kind == 7), (3, kind == 8)):
        keep = np.argsort(rng.random((n, K)), axis=1) < min(want, K)
        drop[rows] = ~keep[rows]
    tab[drop] = 0
    stale = drop & (rng.random((n, K)) < 0.2)                              # count <= 0 with sums left in: empty all the same
    tab[stale, :3] = 12345
    tab[stale & (rng.random((n, K)) < 0.5), 3] = -3
    return tab
