"""Closed-form reconstruction filters: what a set of samples adds to a frame, in plain f64 numpy, as a GATHER.  TESTS ONLY; shared by
tests/test_splat_laws.py (tests/splat_ref.py's restatement and the emulator) and tests/test_gpu_splat_laws.py (vk_splat_* on the device).

Written from the operation's meaning, not from the numbered operation list of include/vecchio_amd.h or from vk_splat.h:
  * pixel (X, Y) covers [X, X + 1) x [Y, Y + 1), its centre is (X + 0.5, Y + 0.5), y is up;
  * the filter is separable; on one axis a sample at p is at d = p - centre from a pixel and in its support iff -r <= d < r;
  * box: 1.  tent: 1 - |d| / r.  Mitchell-Netravali (Mitchell & Netravali, "Reconstruction Filters in Computer Graphics", SIGGRAPH 1988,
    eq. 8) at x = 2 |d| / r:
        6 k(x) = (12 - 9B - 6C) x^3 + (-18 + 12B + 6C) x^2 + (6 - 2B)                   |x| < 1
                 (-B - 6C) x^3 + (6B + 30C) x^2 + (-12B - 48C) x + (8B + 24C)            1 <= |x| < 2
                 0                                                                      otherwise.
gather() visits EVERY pixel of the frame for every sample: no anchor pixel, no window of candidates, no fx - 0.5.  From tests/splat_ref.py
only the shared inputs FILTERS, FRAMES and boundary_positions; from vecchio_amd only the ffi constants that name the three kinds.  The RNG
stream is not under test: where a sample's position is its state's own jitter, the caller passes the draws in.

THE BOUND (derived here, never fitted, never computed from what the restatement, the emulator or the device returns).  u = 2^-24 is the
unit roundoff of f32, g(n) = n u / (1 - n u) the usual bound of n compounded roundings (Higham, Accuracy and Stability, lemma 3.1).  The
position p is an f32 (or an integer plus an f32 draw) and is exact in f64, and so are r, B, C and the radiance a.
  1. Distance.  An f32 evaluation splits p into pixel and fraction exactly (the fraction of an f32 lies on its own grid), subtracts 0.5
     — one rounding of a value of size <= 0.5 — and an integer k, |result| = |d| — one rounding more.  So |d32 - d| <= dd = u (0.5 + |d|)
     (1 + 2u) + slack; `slack` is 0 except where the caller says the positions themselves are only known to within it (case d).
  2. Support.  A (sample, pixel, axis) triple with | |d| - r | <= dd is MARGINAL: f32 may put it on either side.  Every other triple
     falls as in f64.  A pair (sample, pixel) is marginal if one of its triples is and the other is in support or marginal as well.
  3. Per-axis weight, a = |d|.
     BOX: exact.
     TENT: inv_r = fl(1 / r), fl(a32 inv_r) and fl(1 - .): e1 = g(1) |1 - a / r| + (1 + g(1)) (g(2) a / r + (1 + g(2)) dd / r).
     MITCHELL: t32 = fl(a32 fl(2 fl(1 / r))): |t32 - t| <= dt = (1 + g(2)) (2 / r) dd + g(2) t; T = t + dt bounds both.  A cubic in
     Horner form costs at most 6 roundings: the running bound is g(6) sum |c_i| T^i (Higham, section 5.1).  Each of the seven
     coefficients is a sum of at most three terms n_j (12, 9B, 6C, ...) over 6, each term passing through at most 4 roundings (its
     product, two additions, the division): |dc_i| <= g(4) sum_j |n_j| / 6.  Evaluating at t32 instead of t moves the value by at most dt
     sum i |c_i| T^(i - 1).  Together e1 = g(6) sum (|c_i| + |dc_i|) T^i + sum |dc_i| T^i + dt sum i |c_i| T^(i - 1).  Where |t - 1| <=
     dt the f32 side may take the other piece: the two pieces agree in value and slope at 1 (asserted by the self-tests), so they differ
     by at most (6 |p3 - q3| (1 + dt) + |p2 - q2|) dt^2 there, and e1 is the larger of the two pieces' bounds plus that.
  4. Product.  w = fl(wx wy): ew = (|kx| ey + |ky| ex + ex ey) (1 + u) + u |kx ky|.  fl(w a_c): ec = |a_c| ew (1 + u) + u |kx ky a_c|.
     The scaling by 2^26 is exact and the truncation to an integer loses less than one unit: 2^-26 per added value, colour and weight.
  5. A pixel's bound is the sum of (ec + 2^-26) and (ew + 2^-26) over its pairs; a marginal pair adds its full |kx ky a_c| and |kx ky|
     on top (the kernel's formula continued past the support's end, where the pair is outside in f64).  The integer sums are exact.
  6. Resolve.  With C and W the f64 sums and bc, bw their bounds, a pixel is JUDGED when W > bw: then the integer weight sum is
     positive, the two conversions to f32 and the quotient cost g(3), and |out - C / W| <= q + g(3) (|C / W| + q), q = (bc + |C / W| bw) /
     (W - bw).  W < -bw: the resolve is exactly 0.  W = 0 with bw = 0 (nothing reached the pixel): exactly 0.  Everything between is
     unjudged.
Samples here stay below 31.999 in magnitude: the clamp of the sums is not part of this operation."""
import numpy as np

from splat_ref import FILTERS, FRAMES, boundary_positions  # noqa: F401  (shared inputs only)
from vecchio_amd import ffi

f64 = np.float64
BOX, TENT, MITCHELL = ffi.VK_SPLAT_BOX, ffi.VK_SPLAT_TENT, ffi.VK_SPLAT_MITCHELL
U = 2.0 ** -24
UNIT = 2.0 ** -26
MAX_MARGINAL = 1e-3                 # share of the triples in support that may be marginal (case a)
MAX_UNJUDGED = 0.02                 # share of a sparse frame's pixels that may be unjudged (case e)
RADII = (0.5, 0.75, 1.0, 1.25, 1.5, 2.0)


def g(n):
    return n * U / (1.0 - n * U)


# ================================================================ the three published kernels
def mitchell_pieces(B, C):
    """(near, far): the coefficients of x^0 .. x^3 of 6 k on |x| < 1 and on 1 <= |x| < 2, and the |terms| each is a sum of"""
    near = [6.0 - 2.0 * B, 0.0, -18.0 + 12.0 * B + 6.0 * C, 12.0 - 9.0 * B - 6.0 * C]
    far = [8.0 * B + 24.0 * C, -12.0 * B - 48.0 * C, 6.0 * B + 30.0 * C, -B - 6.0 * C]
    near_abs = [6.0 + 2.0 * abs(B), 0.0, 18.0 + 12.0 * abs(B) + 6.0 * abs(C), 12.0 + 9.0 * abs(B) + 6.0 * abs(C)]
    far_abs = [8.0 * abs(B) + 24.0 * abs(C), 12.0 * abs(B) + 48.0 * abs(C), 6.0 * abs(B) + 30.0 * abs(C), abs(B) + 6.0 * abs(C)]
    return near, far, near_abs, far_abs


def _poly(c, x):
    return (c[0] + x * (c[1] + x * (c[2] + x * c[3]))) / 6.0


def mitchell(B, C, x, cut=True):
    """k_{B,C}(x); cut=False continues the outer piece past |x| = 2"""
    x = np.abs(np.asarray(x, f64))
    near, far, _, _ = mitchell_pieces(B, C)
    k = np.where(x < 1.0, _poly(near, x), _poly(far, x))
    return np.where(x < 2.0, k, 0.0) if cut else k


def mitchell_slope(B, C, x, piece):
    """k' of one piece (0 inner, 1 outer) at x >= 0"""
    c = mitchell_pieces(B, C)[piece]
    x = np.asarray(x, f64)
    return (c[1] + x * (2.0 * c[2] + x * 3.0 * c[3])) / 6.0


def tent(x, cut=True):
    x = np.abs(np.asarray(x, f64))
    return np.where(x < 1.0, 1.0 - x, 0.0) if cut else 1.0 - x


def profile(sp, d):
    """the filter's value on one axis at distance d, its formula continued past the support (which in_support() decides)"""
    kind, r, B, C = sp[0], f64(np.float32(sp[1])), f64(np.float32(sp[2])), f64(np.float32(sp[3]))
    d = np.asarray(d, f64)
    if kind == BOX:
        return np.ones_like(d)
    if kind == TENT:
        return 1.0 - np.abs(d) / r
    return mitchell(B, C, 2.0 * np.abs(d) / r, cut=False)


def in_support(sp, d):
    r = f64(np.float32(sp[1]))
    return (d >= -r) & (d < r)


# ================================================================ the bound's per-axis terms
def distance_error(d, slack=0.0):
    return U * (0.5 + np.abs(d)) * (1.0 + 2.0 * U) + slack


def weight_error(sp, d, dd):
    """e1 of the module docstring: how far an f32 evaluation of profile() may lie from the f64 value, given |d32 - d| <= dd"""
    kind, r, B, C = sp[0], f64(np.float32(sp[1])), f64(np.float32(sp[2])), f64(np.float32(sp[3]))
    a = np.abs(np.asarray(d, f64))
    if kind == BOX:
        return np.zeros_like(a)
    if kind == TENT:
        return g(1) * np.abs(1.0 - a / r) + (1.0 + g(1)) * (g(2) * a / r + (1.0 + g(2)) * dd / r)
    t = 2.0 * a / r
    dt = (1.0 + g(2)) * (2.0 / r) * dd + g(2) * t
    T = t + dt
    near, far, near_abs, far_abs = mitchell_pieces(B, C)

    def piece(c, c_abs):
        size = sum(abs(c[i]) / 6.0 * T ** i for i in range(4))
        dc = sum(g(4) * c_abs[i] / 6.0 * T ** i for i in range(4))
        slope = sum(i * abs(c[i]) / 6.0 * T ** (i - 1) for i in range(1, 4))
        return g(6) * (size + dc) + dc + dt * slope

    e_near, e_far = piece(near, near_abs), piece(far, far_abs)
    gap = (6.0 * abs(near[3] - far[3]) * (1.0 + dt) + abs(near[2] - far[2])) / 6.0 * dt * dt
    return np.where(t + dt < 1.0, e_near, np.where(t - dt >= 1.0, e_far, np.maximum(e_near, e_far) + gap))


# ================================================================ the gather
class Stability:
    """what gather() records beside the sums (module docstring, point 2)"""

    def __init__(self):
        self.triples = 0               # (sample, pixel, axis) in support, the other axis reaching the frame
        self.marginal_triples = 0
        self.pairs = 0                 # (sample, pixel) in support on both axes, in f64
        self.marginal_pairs = 0
        self.solid = None              # (height, width): pairs of each pixel that are in support and not marginal

    def marginal_share(self):
        return self.marginal_triples / max(1, self.triples)


class Gathered:
    """sums (height, width, 4) f64: sum w a_r, a_g, a_b and sum w; bound: the same shape; image / image_bound (height, width, 3); judged
    (height, width) bool; black (height, width) bool: the resolve must be exactly 0; abs_weight (height, width): sum |w|; st: the
    Stability record; where asked for, per sample and (height, width): members (the support), maybe (the pairs that may fall either
    way) and weights"""


def _axis(sp, p, extent, slack):
    centre = np.arange(extent, dtype=f64) + 0.5
    d = p[:, None] - centre[None, :]
    dd = distance_error(d, slack)
    r = f64(np.float32(sp[1]))
    inside = in_support(sp, d)
    marginal = np.abs(np.abs(d) - r) <= dd
    k = profile(sp, d)
    e = weight_error(sp, d, dd)
    return inside, marginal, k, e


def gather(sp, positions, radiance, width, height, slack=(0.0, 0.0), members=False):
    """positions (n, 2) f64 frame coordinates, radiance (n, 3): what the samples add to every pixel of a width x height frame"""
    pos = np.asarray(positions, f64).reshape(-1, 2)
    a = np.asarray(radiance, f64).reshape(-1, 3)
    assert np.isfinite(pos).all() and np.isfinite(a).all() and np.abs(a).max(initial=0.0) <= 31.999
    in_x, mg_x, kx, ex = _axis(sp, pos[:, 0], width, slack[0])
    in_y, mg_y, ky, ey = _axis(sp, pos[:, 1], height, slack[1])

    def over(A, B, c=None):            # [Y, X] = sum_n A[n, X] B[n, Y] c[n]
        return (B if c is None else B * c[:, None]).T @ A

    out = Gathered()
    wx, wy = kx * in_x, ky * in_y
    out.sums = np.stack([over(wx, wy, a[:, c]) for c in range(3)] + [over(wx, wy)], axis=-1)
    # every pair an f32 evaluation may add: in support or marginal on both axes; the solid ones among them
    any_x, any_y = in_x | mg_x, in_y | mg_y
    sol_x, sol_y = in_x & ~mg_x, in_y & ~mg_y
    akx, aky = np.abs(kx) * any_x, np.abs(ky) * any_y
    eax, eay = ex * any_x, ey * any_y
    one_x, one_y = any_x.astype(f64), any_y.astype(f64)
    skx, sky = np.abs(kx) * sol_x, np.abs(ky) * sol_y

    def bound(c):                      # c: |a_c| per sample, or None for the weight
        ew = (over(akx, eay, c) + over(eax, aky, c) + over(eax, eay, c)) * (1.0 + U) + U * over(akx, aky, c)
        if c is not None:
            ew = ew * (1.0 + U) + U * over(akx, aky, c)
        return ew + UNIT * over(one_x, one_y) + (over(akx, aky, c) - over(skx, sky, c))

    out.bound = np.stack([bound(np.abs(a[:, c])) for c in range(3)] + [bound(None)], axis=-1)
    out.abs_weight = over(np.abs(wx), np.abs(wy))
    st = Stability()
    st.pairs = int(over(in_x.astype(f64), in_y.astype(f64)).sum())
    st.solid = over(sol_x.astype(f64), sol_y.astype(f64)).astype(np.int64)
    st.marginal_pairs = int(over(one_x, one_y).sum()) - int(st.solid.sum())
    reach_x, reach_y = any_x.any(axis=1), any_y.any(axis=1)
    st.triples = int((in_x & reach_y[:, None]).sum() + (in_y & reach_x[:, None]).sum())
    st.marginal_triples = int((mg_x & reach_y[:, None]).sum() + (mg_y & reach_x[:, None]).sum())
    out.st = st
    if members:
        out.members = in_y[:, :, None] & in_x[:, None, :]
        out.maybe = (any_y[:, :, None] & any_x[:, None, :]) & ~(sol_y[:, :, None] & sol_x[:, None, :])
        out.weights = ky[:, :, None] * kx[:, None, :]
    # the resolve
    W, bw = out.sums[..., 3], out.bound[..., 3]
    out.judged = W > bw
    out.black = (W < -bw) | ((W == 0.0) & (bw == 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(out.judged[..., None], out.sums[..., :3] / W[..., None], 0.0)
        q = (out.bound[..., :3] + np.abs(ratio) * bw[..., None]) / (W - bw)[..., None]
    out.image = ratio
    out.image_bound = np.where(out.judged[..., None], q + g(3) * (np.abs(ratio) + q), np.inf)
    return out


def positions_of_states(pixel, draws, width):
    """a state's own position: its pixel's corner plus the stream's draws 0 (x) and 1 (y), in f64"""
    pixel = np.asarray(pixel, np.int64)
    xi = np.asarray(draws, f64).reshape(-1, 2)
    return np.stack([pixel % width + xi[:, 0], pixel // width + xi[:, 1]], axis=1)


# ================================================================ holding an f32 evaluation to the closed form
def sums_ratio(cf, sums_int):
    """the worst |integer sums x 2^-26 - f64 sums| / bound over a frame (inf where a pixel nothing can reach received something)"""
    got = np.asarray(sums_int, np.int64).astype(f64) * UNIT
    dev = np.abs(got - cf.sums)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(cf.bound > 0.0, dev / cf.bound, np.where(dev > 0.0, np.inf, 0.0))
    return float(ratio.max())


def assert_sums(cf, sums_int, contributions, what):
    """the four sums of every pixel within the bound and the contributions counter within the marginal pairs of the f64 pair count;
    returns the worst ratio"""
    worst = sums_ratio(cf, sums_int)
    assert worst <= 1.0, f"{what}: the sums leave the f64 closed form's bound, ratio {worst:.3g}"
    assert abs(int(contributions) - cf.st.pairs) <= cf.st.marginal_pairs, \
        f"{what}: {contributions} contributions, {cf.st.pairs} pairs in support (+- {cf.st.marginal_pairs} marginal)"
    return worst


def assert_image(cf, image, what):
    """a resolved frame against the closed form's: within the bound where judged, exactly 0 where the weight is surely negative or
    nothing arrived; returns (worst ratio, unjudged share)"""
    img = np.asarray(image, f64).reshape(cf.image.shape)
    assert not img[cf.black].any(), f"{what}: a pixel of negative or no weight is not black"
    with np.errstate(invalid="ignore"):
        ratio = np.where(cf.judged[..., None], np.abs(img - cf.image) / cf.image_bound, 0.0)
    worst = float(ratio.max(initial=0.0))
    assert worst <= 1.0, f"{what}: the resolve leaves the f64 closed form's bound, ratio {worst:.3g}"
    return worst, float((~cf.judged & ~cf.black).mean())
