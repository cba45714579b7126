"""vk_splat_deposit and vk_splat_resolve restated in numpy float32 / int64 from the definition in include/vecchio_amd.h ("reconstruction
filters", points 1 to 5), on top of tests/exact_sums.py and tests/film_ref.py.  The jitter of a sample is draws 0 and 1 of the oracle's
stream of (seed, pixel, sample).  What tests/test_splat_emu.py and tests/test_gpu_splat.py share: the filter settings, the frames and the
positions the deposit is tried on."""
import numpy as np

import exact_sums as E
import film_ref as F
import oracle_ffi
from vecchio_amd import ffi
from vecchio_amd.scene import PATH_STATE_DTYPE

f32 = np.float32
BOX, TENT, MITCHELL = ffi.VK_SPLAT_BOX, ffi.VK_SPLAT_TENT, ffi.VK_SPLAT_MITCHELL
THIRD = float(f32(1.0) / f32(3.0))
# (filter, radius, b, c)
FILTERS = [(BOX, 0.5, 0.0, 0.0), (BOX, 1.0, 0.0, 0.0), (TENT, 1.0, 0.0, 0.0), (TENT, 1.5, 0.0, 0.0),
           (MITCHELL, 2.0, THIRD, THIRD), (MITCHELL, 2.0, 1.0, 0.0), (MITCHELL, 2.0, 0.0, 0.5)]
FILTER_IDS = ["box0.5", "box1", "tent1", "tent1.5", "mitchell", "bspline", "catmull"]
FRAMES = [(21, 13), (1, 1), (3, 2), (64, 5)]         # 1x1 and 3x2: narrower than the footprint
COUNTERS = ("deposited", "dropped", "clamped", "skipped", "contributions")
# (seed, pixel, sample): draw 0 of the first stream and draw 1 of the second are exactly 0.0 — xi = 0, found by search; the tests assert
# it through the oracle
ZERO_X = (0, 0, 12677731)
ZERO_Y = (0, 0, 13705521)

_jitter = {}


def jitter(seed, pixel, sample):
    """(n, 2) float32: draws 0 and 1 of each (seed, pixel, sample)'s stream, from the oracle"""
    out = np.zeros((len(pixel), 2), f32)
    for i, key in enumerate(zip((int(s) for s in seed), (int(p) for p in pixel), (int(s) for s in sample))):
        if key not in _jitter:
            _jitter[key] = oracle_ffi.draws(key[0], key[1], key[2], 0, 2).copy()
        out[i] = _jitter[key]
    return out


def side(radius):
    return int(np.ceil(f32(2.0) * f32(radius)))


def clamp_for(spp, radius):
    """point 4: min(1e10, 1.3e11 / (spp * F)), F = ceil(2 radius)^2"""
    return E.accum_clamp_for(spp * side(radius) ** 2)


def w1(sp, a):
    """point 3: the filter's value at distance a >= 0 on one axis, in f32, in the order the header writes"""
    kind, radius, b, c = sp[0], f32(sp[1]), f32(sp[2]), f32(sp[3])
    a = np.asarray(a, f32)
    if kind == BOX:
        return np.ones_like(a)
    inv_r = f32(1.0) / radius
    if kind == TENT:
        return (f32(1.0) - a * inv_r).astype(f32)
    t = (a * (f32(2.0) * inv_r)).astype(f32)
    p3 = ((f32(12.0) - f32(9.0) * b) - f32(6.0) * c) / f32(6.0)
    p2 = ((f32(-18.0) + f32(12.0) * b) + f32(6.0) * c) / f32(6.0)
    p0 = (f32(6.0) - f32(2.0) * b) / f32(6.0)
    q3 = (-b - f32(6.0) * c) / f32(6.0)
    q2 = (f32(6.0) * b + f32(30.0) * c) / f32(6.0)
    q1 = (f32(-12.0) * b - f32(48.0) * c) / f32(6.0)
    q0 = (f32(8.0) * b + f32(24.0) * c) / f32(6.0)
    assert all(type(v) is f32 for v in (p3, p2, p0, q3, q2, q1, q0))
    near = (((p3 * t + p2) * t) * t + p0).astype(f32)
    far = (((q3 * t + q2) * t + q1) * t + q0).astype(f32)
    return np.where(t < f32(1.0), near, far).astype(f32)


def place(states, status, width, height, positions=None):
    """points 1 and 2: (placed, ix, iy, fx, fy) per candidate"""
    n = len(states)
    retired = np.isin(status, F.DEPOSITING)
    ix, iy = np.zeros(n, np.int64), np.zeros(n, np.int64)
    fx, fy = np.zeros(n, f32), np.zeros(n, f32)
    if positions is None:
        pixel = states["pixel"].astype(np.int64)
        placed = retired & (pixel < width * height)
        ix[placed], iy[placed] = pixel[placed] % width, pixel[placed] // width
        j = jitter(states["seed"][placed], states["pixel"][placed], states["sample"][placed])
        fx[placed], fy[placed] = j[:, 0], j[:, 1]
    else:
        pos = np.asarray(positions, f32).reshape(n, 2)
        with np.errstate(invalid="ignore"):
            fl = np.floor(pos).astype(f32)
            ok = np.isfinite(pos).all(axis=1) & (fl[:, 0] >= 0) & (fl[:, 0] < width) & (fl[:, 1] >= 0) & (fl[:, 1] < height)
        placed = retired & ok
        ix[placed], iy[placed] = fl[placed, 0].astype(np.int64), fl[placed, 1].astype(np.int64)
        fx[placed], fy[placed] = (pos[placed, 0] - fl[placed, 0]).astype(f32), (pos[placed, 1] - fl[placed, 1]).astype(f32)
    return placed, ix, iy, fx, fy


def deposit(states, status, width, height, spp, sp, positions=None, sums=None):
    """vk_splat_deposit in numpy: (sums (height, width, 4) int64 — added to where given —, dict of the five device counters)"""
    states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1)
    status = np.ascontiguousarray(status, np.uint32).reshape(-1)
    sums = np.zeros((height, width, 4), np.int64) if sums is None else sums.copy()
    flat = sums.reshape(width * height, 4)
    radius = f32(sp[1])
    placed, ix, iy, fx, fy = place(states, status, width, height, positions)
    acc = states["acc"].astype(f32)
    finite = np.isfinite(acc).all(axis=1)
    dep = placed & finite
    clampv = clamp_for(spp, sp[1])
    with np.errstate(invalid="ignore"):
        big = np.abs(acc).max(axis=1)
        large = big > E.ACCUM_SMALL
        a = np.where(large[:, None], np.clip(acc, -clampv, clampv), acc).astype(f32)
    contributions = 0
    cx, cy = (fx - f32(0.5)).astype(f32), (fy - f32(0.5)).astype(f32)
    for ky in range(-2, 3):
        dy = (cy - f32(ky)).astype(f32)
        in_y = (dy >= -radius) & (dy < radius) & (iy + ky >= 0) & (iy + ky < height)
        wy = w1(sp, np.abs(dy))
        for kx in range(-2, 3):
            dx = (cx - f32(kx)).astype(f32)
            sel = dep & in_y & (dx >= -radius) & (dx < radius) & (ix + kx >= 0) & (ix + kx < width)
            if not sel.any():
                continue
            w = (w1(sp, np.abs(dx)) * wy).astype(f32)[sel]
            vals = np.empty((int(sel.sum()), 4), np.int64)
            vals[:, :3] = np.trunc((w[:, None] * a[sel]).astype(f32) * E.ACCUM_SCALE).astype(np.int64)
            vals[:, 3] = np.trunc(w * E.ACCUM_SCALE).astype(np.int64)
            np.add.at(flat, ((iy + ky) * width + ix + kx)[sel], vals)
            contributions += int(sel.sum())
    counters = dict(deposited=int(dep.sum()), dropped=int((placed & ~finite).sum()),
                    clamped=int((dep & large & (big > clampv)).sum()), skipped=int((~placed).sum()), contributions=contributions)
    return sums, counters


def resolve(sums4):
    """point 5: rgb = w_sum > 0 ? ((float)c_sum * 2^-26) / ((float)w_sum * 2^-26) : 0"""
    s = np.asarray(sums4, np.int64)
    inv = f32(1.0 / 2.0 ** 26)
    w = s[..., 3].astype(f32) * inv
    c = s[..., :3].astype(f32) * inv
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (c / w[..., None]).astype(f32)
    return np.where((s[..., 3] > 0)[..., None], out, f32(0.0)).astype(f32)


def counters_of(info):
    return {k: int(getattr(info, k)) for k in COUNTERS}


def anchors(width, height):
    """pixels in all four corners, on every edge and inside (deduplicated on frames narrower than that)"""
    xs, ys = sorted({0, width // 2, width - 1}), sorted({0, height // 2, height - 1})
    return np.array([y * width + x for y in ys for x in xs], np.uint32)


def states_with_samples(pixel, acc, seed=0):
    """film_ref.states_for with a sample number of its own per state: every state its own jitter"""
    st = F.states_for(pixel, acc, seed)
    st["sample"] = np.arange(len(pixel)) % 97
    return st


def boundary_positions(width, height):
    """(n, 2) float32 frame coordinates: on pixel boundaries, at -0.0, just inside and exactly at `width` / `height` (skipped), negative,
    NaN and infinite (skipped), and ordinary ones"""
    W, H = f32(width), f32(height)
    below = lambda v: np.nextafter(f32(v), f32(-1))
    pts = [(0.0, 0.0), (-0.0, -0.0), (-0.0, 0.5), (1.0, 1.0), (0.5, 0.5), (below(W), below(H)), (W, 0.5), (0.5, H), (W, H),
           (below(0.0), 0.5), (0.5, -1.0), (np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (0.5, -np.inf), (W - f32(1), H - f32(1)),
           (W * f32(0.5), H * f32(0.5)), (0.25, below(H)), (below(W), 0.75), (below(1.0), below(1.0)), (3.0e9, 0.5), (1e-30, 1e-30)]
    rng = np.random.default_rng(width * 1000 + height)
    rand = (rng.random((40, 2)) * np.array([width, height])).astype(f32)
    rand = np.minimum(rand, np.array([below(W), below(H)], f32))
    return np.concatenate([np.array(pts, f32), rand])
