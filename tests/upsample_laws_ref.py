"""The laws of guided upsampling (vk_upsample_*), in f64, written from what the operator MEANS — a normalised weighted mean of low pixels
under a tent of half-width two low pixels, with weights that vanish across an edge of the guides — and not from its code.  Each law is a
function of an `apply` with upsample_ref.apply's signature, so the same checks run on the numpy restatement, on the host build and on the
device.  TESTS ONLY.

The bounds.  u = 2^-24 is the unit roundoff of f32 and g(n) = n u / (1 - n u) bounds n compounded roundings (Higham, Accuracy and Stability
of Numerical Algorithms, lemma 3.1).  out_c = fl(fl(J_c / Wt) A_c) with J_c = sum wt_i I_i and Wt = sum wt_i over at most 16 taps, the
SAME floats wt_i in both sums, so an error of a weight cancels wherever every I_i is the same number.
  J:  one product and at most 15 additions per term, non-negative terms: relative error g(16).
  Wt: at most 15 additions: g(15).  The division: 1.  The product with A_c: 1 (0 where A_c = 1).
  A weight may be subnormal (E falls to 0 smoothly); its product then carries an absolute error of 2^-150, and with Wt >= 1e-4 the 16 of
  them move the result by less than 2^-132: DENORMAL_SLACK covers it.
(a), (c): a constant (on the pixel's side): g(16) + g(15) + 1 u -> BOUND_CONSTANT = g(32) = 32.0001 u relative.
(d): the input colour fl(L a) (1), the demodulation fl(c / a) (1), the constant law (32), the product with A (1): g(35) = 35.0001 u.
(b): an affine frame v(x, y) = v0 + bx x + by y with values exact in f32.  Three parts, absolute:
  the sums, as above: every term of J is positive, so its error is g(16) of J itself, and the whole is g(32) |v|;
  the weights.  kx~ = fl(1 - fl(|fl(px~ - tx)| 0.5)): the difference of two floats below 2^23 with |d| < 2 errs by at most u |d| <= 2 u,
    halved exactly, and 1 - . rounds once more (<= u): |kx~ - tent(px~ - tx)| <= 2 u; the product kx~ ky~ adds u kx ky.  A weight's
    error moves the mean only through (I_i - v(px~, py~)), at most 2 |bx| + 2 |by| inside the footprint, so the mean moves by at most
    sum_i |dk_i| (2 |bx| + 2 |by|) / Wt with sum_i |dk_i| <= 2 u (4 sum ky + 4 sum kx) + u sum kx ky = 36 u and Wt = 4: 9 u (2 |bx| + 2 |by|);
  the centre.  px~ = fl(fl((X + 0.5) rx~) - 0.5) with rx~ = fl(rx): |px~ - px| <= 3 u (|px| + 0.5); the tent reproduces v at px~, so
    the value moves by |bx| 3 u (|px| + 0.5) + |by| 3 u (|py| + 0.5).
  Relative to |v| on the shapes and the frame the tests use the sum is at most LINEAR_WORST = 48.1 u (test_upsample_laws.py asserts that).
(e): no rounding bound: a chi-square interval (below)."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
DENORMAL_SLACK = 2.0 ** -130
# the shapes laws (a), (b) and (c) were first checked on
SHAPES = [(7, 5, 16, 11), (8, 6, 16, 12), (5, 4, 37, 29), (9, 7, 9, 7), (2, 2, 5, 5), (9, 7, 31, 23)]


def g(n):
    return n * U / (1.0 - n * U)


BOUND_CONSTANT = g(32)
BOUND_DEMODULATION = g(35)
LINEAR_WORST = 48.1 * U


def centres(lo, hi):
    """where the centre of each high pixel of one axis lies in low pixels: the frame convention, pixel x covers u in [x / (n - 1),
    (x + 1) / (n - 1)], so a centre (X + 0.5) / (hi - 1) is low coordinate (X + 0.5) (lo - 1) / (hi - 1) - 0.5"""
    return (np.arange(hi, dtype=f64) + 0.5) * (f64(lo - 1) / f64(hi - 1)) - 0.5


def interior(w, h, W, H):
    """the high pixels whose 4 x 4 footprint lies inside the low image"""
    fx, fy = np.floor(centres(w, W)), np.floor(centres(h, H))
    return ((fy >= 1) & (fy + 2 <= h - 1))[:, None] & ((fx >= 1) & (fx + 2 <= w - 1))[None, :]


def rough_guides(n_x, n_y, seed):
    """a normal and a depth image that say nothing in particular: unit-ish normals that vary, a depth with ramps and noise"""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(n_y, n_x, 3)) + np.array([0.0, 0.0, 2.5])
    z = 2.0 + rng.random((n_y, n_x)) * 0.01 + 0.3 * np.arange(n_x)[None, :] / n_x
    return n.astype(f32), z.astype(f32)


def law_constant(apply, shape, value=0.7):
    """(a) a constant low frame gives the constant, whatever the guides: no guides, a normal and a depth that vary from pixel to pixel,
    each alone and both.  Returns the worst relative error in units of u."""
    w, h, W, H = shape
    c = np.full((h, w, 3), value, f32)
    want = f64(f32(value))
    n, z = rough_guides(w, h, 11)
    N, Z = rough_guides(W, H, 12)
    worst = 0.0
    for kw in ({}, dict(normal=n, normal_hi=N), dict(depth=z, depth_hi=Z), dict(normal=n, normal_hi=N, depth=z, depth_hi=Z),
               dict(normal=n, normal_hi=N, depth=z, depth_hi=Z, sigma_z=0.5, normal_squarings=3)):
        out, _, _, empty = apply(c, W, H, want_stderr=False, **kw)
        assert empty == 0
        err = np.abs(out.astype(f64) - want).max() / want
        assert err <= BOUND_CONSTANT + DENORMAL_SLACK, (shape, sorted(kw), err / U)
        worst = max(worst, err)
    return worst / U


LINEAR = (0.25, 0.5, 0.125)        # v0, bx, by: every value of the low frame is exact in f32


def linear_bound(shape):
    """(tolerance (H, W), the affine function at the high centres (H, W)) of law (b)"""
    w, h, W, H = shape
    v0, bx, by = LINEAR
    px, py = centres(w, W)[None, :], centres(h, H)[:, None]
    v = v0 + bx * px + by * py
    tol = g(32) * np.abs(v) + 9 * U * (2 * abs(bx) + 2 * abs(by)) + 3 * U * (abs(bx) * (np.abs(px) + 0.5) + abs(by) * (np.abs(py) + 0.5))
    return tol * (1 + 64 * U), v


def law_linear(apply, shape):
    """(b) a low frame affine in (x, y), under flat guides, gives the affine function at the high pixel's centre wherever the 4 x 4
    footprint lies inside the low image: the tent's weights sum to 2 and have zero first moment at any phase.  Returns (interior pixels,
    the worst error over its tolerance, the worst relative error in units of u)."""
    w, h, W, H = shape
    v0, bx, by = LINEAR
    lo = (v0 + bx * np.arange(w, dtype=f64)[None, :] + by * np.arange(h, dtype=f64)[:, None])
    assert (lo.astype(f32).astype(f64) == lo).all()
    c = np.repeat(lo.astype(f32)[..., None], 3, -1)
    m = interior(*shape)
    tol, v = linear_bound(shape)
    flat_n = np.tile(np.array([0.0, 0.0, 1.0], f32), (h, w, 1)), np.tile(np.array([0.0, 0.0, 1.0], f32), (H, W, 1))
    flat_z = np.full((h, w), 2.5, f32), np.full((H, W), 2.5, f32)
    worst = rel = 0.0
    for kw in ({}, dict(normal=flat_n[0], normal_hi=flat_n[1], depth=flat_z[0], depth_hi=flat_z[1])):
        out, _, fb, _ = apply(c, W, H, want_stderr=False, **kw)
        assert fb == 0
        err = np.abs(out.astype(f64) - v[..., None]).max(-1)
        if m.any():
            assert (err[m] <= tol[m]).all(), (shape, sorted(kw), (err[m] / tol[m]).max())
            worst, rel = max(worst, (err[m] / tol[m]).max()), max(rel, (err[m] / np.abs(v[m])).max())
    return int(m.sum()), worst, rel / U


EDGE_U, EDGE_NEAR, EDGE_FAR = 0.47, (1.0, 0.2), (3.0, 5.0)        # the edge; (depth, value) left of it and right of it


def edge_side(n):
    """True where a pixel of an n-wide frame lies left of the edge: its centre is at u = (x + 0.5) / (n - 1)"""
    return (np.arange(n) + 0.5) / (n - 1) < EDGE_U


def law_edges(apply, shape=(9, 7, 31, 23)):
    """(c) two surfaces at depths 1 and 3 with values 0.2 and 5.0 meet at a vertical edge at u = 0.47; the depth is sampled at both
    sizes.  Every high pixel gets its own side's value within the constant law's bound, and none falls back.  POWER: without the guides
    the same frame is off by more than 1 near the edge.  Returns (worst relative error in u, worst error without guides)."""
    w, h, W, H = shape
    sl, sh = edge_side(w), edge_side(W)
    assert sl.any() and not sl.all() and sh.any() and not sh.all()
    zlo = np.where(sl, EDGE_NEAR[0], EDGE_FAR[0])[None, :] * np.ones((h, 1))
    zhi = np.where(sh, EDGE_NEAR[0], EDGE_FAR[0])[None, :] * np.ones((H, 1))
    val = np.where(sl, EDGE_NEAR[1], EDGE_FAR[1])[None, :] * np.ones((h, 1))
    c = np.repeat(val.astype(f32)[..., None], 3, -1)
    want = np.where(sh, f64(f32(EDGE_NEAR[1])), f64(f32(EDGE_FAR[1])))[None, :, None] * np.ones((H, 1, 3))
    out, _, fb, empty = apply(c, W, H, depth=zlo.astype(f32), depth_hi=zhi.astype(f32), want_stderr=False)
    assert fb == 0 and empty == 0, (shape, fb, empty)
    err = (np.abs(out.astype(f64) - want) / want).max()
    assert err <= BOUND_CONSTANT + DENORMAL_SLACK, (shape, err / U)
    plain, _, _, _ = apply(c, W, H, want_stderr=False)
    off = np.abs(plain.astype(f64) - want).max()
    assert off > 1.0, off
    return err / U, off


def law_demodulation(apply, shape=(8, 6, 16, 12), irradiance=1.7):
    """(d) constant irradiance under a checker albedo at the high size and its average at the low size: the output is irradiance x
    albedo_hi.  Returns the worst relative error in units of u."""
    w, h, W, H = shape
    chk = ((np.arange(W)[None, :] + np.arange(H)[:, None]) % 2).astype(bool)
    A = np.where(chk[..., None], np.array([0.8, 0.6, 0.9]), np.array([0.2, 0.3, 0.1])).astype(f32)
    a = np.broadcast_to(A.astype(f64).reshape(-1, 3).mean(0), (h, w, 3)).astype(f32)
    c = (f64(irradiance) * a.astype(f64)).astype(f32)
    out, _, fb, _ = apply(c, W, H, albedo=a, albedo_hi=A, want_stderr=False)
    assert fb == 0
    want = f64(irradiance) * A.astype(f64)
    err = (np.abs(out.astype(f64) - want) / want).max()
    assert err <= BOUND_DEMODULATION, (shape, err / U)
    return err / U


# (e) the variance.  n = VAR_DRAWS independent low frames, every pixel N(mean, sigma^2); the reported stderr3_out of an interior pixel is
# the same number r in every draw (the weights do not depend on the colour), and if it is the output's true standard deviation then
# (n - 1) s^2 / r^2 is chi-square with n - 1 degrees of freedom.  Laurent and Massart (2000, lemma 1): P(chi2_k >= k + 2 sqrt(k x) + 2 x)
# <= e^-x and P(chi2_k <= k - 2 sqrt(k x)) <= e^-x.  With VAR_TESTS pixel-components judged, two sides each, and a false-alarm rate of
# VAR_ALPHA for the whole law, x = ln(2 VAR_TESTS / VAR_ALPHA).  POWER: a stderr3_out too large by 1.5 divides the statistic by 2.25; its
# mean k / 2.25 = 355 then lies 11 of its standard deviations (sqrt(2 k) / 2.25 = 17.8) below the lower limit 560, so it is rejected.
VAR_DRAWS, VAR_TESTS, VAR_ALPHA, VAR_SIGMA, VAR_MEAN = 800, 27, 1e-6, 0.25, 3.0
VAR_SHAPE = (8, 6, 16, 12)


def chi2_interval(k, tests=VAR_TESTS, alpha=VAR_ALPHA):
    x = math.log(2 * tests / alpha)
    return k - 2 * math.sqrt(k * x), k + 2 * math.sqrt(k * x) + 2 * x


def variance_draws():
    """the VAR_DRAWS low frames (n, h, w, 3) f32 and their stderr3 (h, w, 3)"""
    w, h, _, _ = VAR_SHAPE
    rng = np.random.default_rng(20071)
    return (VAR_MEAN + VAR_SIGMA * rng.standard_normal((VAR_DRAWS, h, w, 3))).astype(f32), np.full((h, w, 3), VAR_SIGMA, f32)


def law_variance(outputs, reported):
    """(e) outputs (n, H, W, 3): the upsampled draws; reported (H, W, 3): stderr3_out (of any draw).  The spread of VAR_TESTS interior
    pixel-components agrees with what is reported, and does not with 1.5 times it.  Returns the statistics over k."""
    w, h, W, H = VAR_SHAPE
    m = np.argwhere(interior(*VAR_SHAPE))
    assert len(m) * 3 >= VAR_TESTS
    pick = m[np.linspace(0, len(m) - 1, VAR_TESTS // 3).astype(int)]
    k = VAR_DRAWS - 1
    lo, hi = chi2_interval(k)
    o = np.asarray(outputs, f64)
    stats = []
    for y, x in pick:
        for ch in range(3):
            r = f64(reported[y, x, ch])
            t = k * o[:, y, x, ch].var(ddof=1) / (r * r)
            assert lo <= t <= hi, ((y, x, ch), t, lo, hi)
            assert not lo <= t / 2.25 <= hi, ("power", (y, x, ch), t / 2.25, lo, hi)
            stats.append(t / k)
    assert len(stats) == VAR_TESTS
    return stats
