"""What the library's error estimates and stopping rules MEAN, against a fully known sample law.  TESTS ONLY; shared by
tests/test_estimator_laws.py (oracle, emulator, and this module against itself) and tests/test_gpu_estimator_laws.py (the public calls).

Everything here is plain f64 numpy.  It imports tests/radiometry_ref.py for the scene and nothing from adaptive_ref.py, adapt_ref.py,
robust_ref.py or temporal_ref.py: those restate the formulas of the calls under test, and a wrong restatement (k for k - 1, a window
weighted by n_j^2, a variance where a standard error is expected) is wrong on the device and in numpy together.  What is written here
comes from include/vecchio_amd.h's WORDS ("the batch-means standard error of the current mean", "a tile converges when ...", the seven
resolve steps) and from the law below.

The law.  In the integrating sphere's frame (radiometry_ref.sphere_scene / sphere_camera, SCATTER integrator) every pixel sees the wall,
and segment 2, 3, ... of a path meets the lamp with probability f = SPHERE_F = 1/4 each.  With max_depth = D a sample is
    Y_c = Le_c a_c^j   with probability f (1 - f)^(j - 1),  j = 1 .. D - 1   (the same j in all three channels),
    Y   = 0            otherwise, with probability (1 - f)^(D - 1).
Every pixel of a frame is an independent draw from it: mu, sigma^2 and every higher moment are finite geometric sums.

The rules (|z| <= Z_MAX = 4 throughout, every SE from the data's own spread, every SE capped so that no pass is vacuous):
  A  variance:  R_c = mean over pixels of stderr_c^2 / (sigma_c^2 / N);  |R - 1| <= 4 SE.
  B  coverage:  the share of pixels with |mean_c - mu_c| <= 2 stderr_c, per channel, against the share the same plan gives on draw();
  C  stopping:  the mean tile count against a simulation of the header's rule on draw();
  D  robust:    the frame's mean of rgb / mu and of stderr^2 N / sigma^2 against a simulation of the header's resolve steps on draw();
  E  temporal:  rule A for out_stderr3 and the pixels' spread of out_color against sigma^2 / (64 n).
Every rule has power controls: plausible wrong restatements whose expectation the same data must reject by |z| > 4.

Measured figures: see MEASURED at the end of this module."""
import functools
import math

import numpy as np

import radiometry_ref as R

f64, f32 = np.float64, np.float32
Z_MAX = 4.0
A, LE, F = np.asarray(R.SPHERE_A, f64), np.asarray(R.SPHERE_LE, f64), float(R.SPHERE_F)
SEED = R.SPHERE_SEED
DEPTHS = (3, 50)
SIM_SEED = 20240611                     # numpy's generator for every simulation here: PCG64(SIM_SEED + a per-use offset)


# ================================================================ the law
class Law:
    """values[j - 1] = Le a^j (D - 1 of them, 3 channels), probs[j - 1] = f (1 - f)^(j - 1), p_zero = (1 - f)^(D - 1); mu, second
    moment m2 and variance var per channel as plain sums over the table"""

    def __init__(self, D):
        assert D >= 2
        self.D = D
        self.j = np.arange(1, D)
        self.values = LE * A ** self.j[:, None].astype(f64)
        self.probs = F * (1.0 - F) ** (self.j - 1.0)
        self.p_zero = (1.0 - F) ** (D - 1)
        self.mu = (self.probs[:, None] * self.values).sum(0)
        self.m2 = (self.probs[:, None] * self.values ** 2).sum(0)
        self.var = self.m2 - self.mu ** 2
        self.table = np.vstack([np.zeros((1, 3)), self.values])          # row 0: the zero sample; row j: Le a^j

    def draw_j(self, rng, shape):
        """j per sample from numpy's own generator: geometric(f) on 1, 2, ..; a j beyond D - 1 is the zero sample, coded 0"""
        j = rng.geometric(F, size=shape)
        return np.where(j < self.D, j, 0).astype(np.uint8)

    def draw(self, rng, shape):
        """samples of the given shape + (3,)"""
        return self.table[self.draw_j(rng, shape)]

    def closed_forms(self):
        """(mu, E[Y^2]) as the geometric sums in closed form: mu = a Le f (1 - q^(D-1)) / (1 - q), q = a (1 - f) (radiometry_ref's
        integrating_sphere with one segment spent on the way to the wall); E[Y^2] = f Le^2 a^2 (1 - r^(D-1)) / (1 - r), r = a^2 (1 - f)"""
        n = self.D - 1
        r = A * A * (1.0 - F)
        return A * R.integrating_sphere(A, F, LE, n), F * LE ** 2 * A ** 2 * (1.0 - r ** n) / (1.0 - r)


@functools.lru_cache(None)
def law(D):
    return Law(D)


def rng_for(*key):
    return np.random.Generator(np.random.PCG64([SIM_SEED, *[int(k) for k in key]]))


def window_sums(lw, rng, pixels, windows, chunk=1 << 13):
    """(pixels, k, 3): per pixel the sum of each window's samples, windows = (n_1 .. n_k), drawn pixel chunk by pixel chunk"""
    out = np.empty((pixels, len(windows), 3), f64)
    for p0 in range(0, pixels, chunk):
        p1 = min(pixels, p0 + chunk)
        for w, n in enumerate(windows):
            out[p0:p1, w] = lw.draw(rng, (p1 - p0, n)).sum(1)
    return out


# ================================================================ A: the batch-means variance
# (width, height, windows) and the cap on R's SE — a condition, not a measurement
PLANS = {
    "equal":   (32, 32, (64, 64, 64, 64), 0.03),
    "unequal": (32, 32, (16, 48, 64, 128), 0.03),
    "k8":      (64, 64, (32,) * 8, 0.01),
    "k2":      (32, 32, (8, 8), 0.05),
    # two larger frames of the same windows, for rule B's control (control_power_b): the caps scale with 1 / sqrt(pixels)
    "equal64": (64, 64, (64, 64, 64, 64), 0.015),
    "k8_128":  (128, 128, (32,) * 8, 0.005),
}


def batch_means(sums, windows):
    """(mean, stderr^2), each (pixels, 3), of window sums (pixels, k, 3): the header's words for vk_progress_stderr — "(sum_j n_j m_j^2 -
    N m^2) / ((k - 1) N) with k the steps, n_j and m_j window j's length and own mean, N = samples_done and m the running mean".  This
    is what the SIMULATIONS of rules B and C apply to draw(); rule A's expectation is sigma^2 / N, which needs none of it."""
    n = np.asarray(windows, f64)
    N, k = n.sum(), len(n)
    m_j = sums / n[:, None]
    m = sums.sum(1) / N
    return m, ((n[:, None] * m_j ** 2).sum(1) - N * m ** 2) / ((k - 1) * N)


def ratio(per_pixel):
    """(mean, SE from the pixels' spread) per channel of a per-pixel statistic (pixels, 3)"""
    x = np.asarray(per_pixel, f64).reshape(-1, 3)
    return x.mean(0), x.std(0, ddof=1) / math.sqrt(len(x))


def rule_a(stderr, var_of_mean, se_cap, what, controls=()):
    """rule A for a stderr image (.., 3) whose squares should average var_of_mean (3,); controls: factors c != 1 such that a wrong
    estimator would average c * var_of_mean.  Returns (R, SE, z, z of each control)."""
    r, se = ratio(np.asarray(stderr, f64).reshape(-1, 3) ** 2 / var_of_mean)
    z = (r - 1.0) / se
    assert (se <= se_cap).all(), f"{what}: SE {se} above its cap {se_cap}: the comparison would be vacuous"
    assert (np.abs(z) <= Z_MAX).all(), f"{what}: mean of stderr^2 / (sigma^2 / N) = {r}, se {se}, z {z}"
    zc = [(r - c) / se for c in controls]
    for c, zz in zip(controls, zc):
        assert (np.abs(zz) > Z_MAX).all(), f"{what}: the power control {c} is not rejected: R {r} se {se} z {zz}"
    return r, se, z, zc


def control_divisor_k(windows):
    """the divisor k for k - 1: (k - 1) / k of the variance"""
    k = len(windows)
    return (k - 1.0) / k


def control_equal_weights(windows):
    """window means weighted equally: sum_j (m_j - mean_j m_j)^2 / (k (k - 1)), whose expectation is sigma^2 (1 / k^2) sum_j 1 / n_j:
    N / k^2 * sum_j 1 / n_j of sigma^2 / N (1 for equal windows, 1.708 for 16, 48, 64, 128)"""
    n = np.asarray(windows, f64)
    return n.sum() / len(n) ** 2 * (1.0 / n).sum()


# ================================================================ B: coverage
COVER_PIXELS = 1 << 18


def covered(mean, stderr, mu, scale=1.0):
    """per channel the share of pixels with |mean - mu| <= 2 * scale * stderr"""
    mean, stderr = np.asarray(mean, f64).reshape(-1, 3), np.asarray(stderr, f64).reshape(-1, 3)
    return (np.abs(mean - mu) <= 2.0 * scale * stderr).mean(0)


COVER_SUB = 16                          # the three plans of 256 samples are all made of sub-windows of 16: one draw serves them


@functools.lru_cache(None)
def _coverage_table(D, N):
    """{windows: (share, share if stderr were sqrt(k / (k - 1)) times too small)} per channel, for every plan of N samples, over
    COVER_PIXELS pixels of draw().  Plans of the same N regroup the same sub-window sums; each is a valid draw of its own plan."""
    lw = law(D)
    todo = sorted({pl[2] for pl in PLANS.values() if sum(pl[2]) == N})
    sub = math.gcd(COVER_SUB, *[n for w in todo for n in w])
    out = {w: [np.zeros(3), np.zeros(3)] for w in todo}
    rng = rng_for(2, D, N)
    chunk = 1 << 14
    for p0 in range(0, COVER_PIXELS, chunk):
        s = window_sums(lw, rng, chunk, (sub,) * (N // sub), chunk)
        for w in todo:
            edges = np.cumsum((0,) + w) // sub
            g = np.stack([s[:, a:b].sum(1) for a, b in zip(edges[:-1], edges[1:])], 1)
            mean, v = batch_means(g, w)
            se = np.sqrt(np.maximum(v, 0.0))
            k = len(w)
            out[w][0] += covered(mean, se, lw.mu) * chunk / COVER_PIXELS
            out[w][1] += covered(mean, se, lw.mu, math.sqrt((k - 1.0) / k)) * chunk / COVER_PIXELS
    return {w: tuple(v) for w, v in out.items()}


def coverage_expected(D, plan):
    """(share, the control's share) per channel under the plan's windows.  The sample mean is far from normal at these N (at D = 3 a
    sample takes three values), so no t quantile stands in: the expectation is the same plan on draw()."""
    windows = PLANS[plan][2]
    return _coverage_table(D, sum(windows))[windows]


POWER_MIN = 6.0                         # a control is asked of a run only where it lies this many SE away: 2 SE of room over Z_MAX


def control_power_b(D, plan, pixels):
    """how many binomial SE (at `pixels` pixels) the control's share lies from the expected one, per channel"""
    want, ctrl = coverage_expected(D, plan)
    return np.abs(want - ctrl) / np.sqrt(ctrl * (1.0 - ctrl) * (1.0 / pixels + 1.0 / COVER_PIXELS))


def rule_b(mean, stderr, D, plan, what):
    """the share against the simulation's, per channel, within 4 binomial SE (both sides' counts).  Per channel and not over (pixel,
    channel) pairs pooled: the three channels of a pixel share every j, so pooled pairs are not independent trials and their binomial
    SE would be too small by up to sqrt(3).
    The control — the share expected if stderr were sqrt(k / (k - 1)) times too small — is 4 to 5 points of coverage away at k = 4 and
    2 at k = 8: 3.5 binomial SE of a 1024-pixel (k = 4) or 4096-pixel (k = 8) frame, which such a frame cannot reject at 4.  It is
    asserted where control_power_b() >= POWER_MIN: the k = 2 plan (green and blue), and the plans 'equal64' and 'k8_128', the same
    windows on four times the pixels, which exist for this.  Returns (share, expected, z, control's share, z against it, asked)."""
    lw = law(D)
    want, ctrl = coverage_expected(D, plan)
    got = covered(mean, stderr, lw.mu)
    n = np.asarray(mean).reshape(-1, 3).shape[0]
    se = lambda p: np.sqrt(p * (1.0 - p) * (1.0 / n + 1.0 / COVER_PIXELS))
    z, zc = (got - want) / se(want), (got - ctrl) / se(ctrl)
    assert (np.abs(z) <= Z_MAX).all(), f"{what}: covered {got}, expected {want}, z {z}"
    asked = control_power_b(D, plan, n) >= POWER_MIN
    assert (np.abs(zc[asked]) > Z_MAX).all(), f"{what}: the control's share {ctrl} is not rejected: covered {got}, z {zc}, asked of {asked}"
    return got, want, z, ctrl, zc, asked


# ================================================================ C: the stopping rule
STOP = dict(D=50, window=32, budget=1024, abs_tol=0.0, rel_tol=0.2, min_samples=64, min_steps=2)
STOP_TILES = 2048


@functools.lru_cache(None)
def simulate_stopping(tw, th, tiles=STOP_TILES, divisor_k=False):
    """The header's rule on draw(), for `tiles` independent tiles of tw x th in-image pixels: after every window of STOP['window'] samples
    "a pixel has converged when for every component c  v_c <= (abs_tol + rel_tol |mean_c|)^2", v_c the variance vk_progress_stderr
    squares at N = samples_done and k = steps; "a tile converges when all its in-image pixels have, with N >= min_samples and k >=
    min_steps"; a converged tile is frozen; nothing goes beyond the budget.  divisor_k: the control, v_c with k for k - 1.
    Returns (count per tile, per tile the mean over its pixels of frozen mean / mu)."""
    s = STOP
    lw = law(s["D"])
    rng = rng_for(3, tw, th, tiles, int(divisor_k))
    n = s["window"]
    tol = f64(f32(s["rel_tol"]))                    # the parameter is a float in vk_adaptive_params
    px = tw * th
    run, m2 = np.zeros((tiles, px, 3)), np.zeros((tiles, px, 3))
    count, bias = np.zeros(tiles, np.int64), np.zeros((tiles, 3))
    active = np.arange(tiles)
    N = k = 0
    while len(active) and N + n <= s["budget"]:
        w = np.empty((len(active), px, 3))
        for t0 in range(0, len(active), 256):
            w[t0:t0 + 256] = lw.draw(rng, (len(active[t0:t0 + 256]), px, n)).sum(2)
        run[active] += w
        m2[active] += w * w / n
        N, k = N + n, k + 1
        mean = run[active] / N
        if k >= 2:
            v = (m2[active] - N * mean * mean) / ((k if divisor_k else k - 1) * N)
            done = (v <= (s["abs_tol"] + tol * np.abs(mean)) ** 2).all((1, 2)) & (N >= s["min_samples"]) & (k >= s["min_steps"])
        else:
            done = np.zeros(len(active), bool)
        if N + n > s["budget"]:
            done[:] = True                          # the budget ends the rest
        count[active[done]] = N
        bias[active[done]] = (mean[done] / lw.mu).mean(1)
        active = active[~done]
    return count, bias


def tile_shapes(width, height):
    """{(tw, th): boolean (tiles_y, tiles_x) mask} of an image's 8 x 8 tiling, tile row 0 at the bottom: "only a partial tile's in-image
    pixels are judged" — tw = min(8, W - 8 tx), th = min(8, H - 8 ty)"""
    tx, ty = (width + 7) // 8, (height + 7) // 8
    tw = np.minimum(8, width - 8 * np.arange(tx))[None, :].repeat(ty, 0)
    th = np.minimum(8, height - 8 * np.arange(ty))[:, None].repeat(tx, 1)
    return {(int(a), int(b)): (tw == a) & (th == b) for a, b in sorted(set(zip(tw.ravel(), th.ravel())))}


def rule_c(tile_samples, width, height, what, own_spread_from=16):
    """the device's mean tile count per tile shape against the simulation's, within 4 combined SE; the control (k for k - 1) rejected
    for whole tiles where there are at least `own_spread_from` of them.  The device side's SE is its tiles' own spread where a shape
    has that many tiles, else the simulation's spread (the same law) over the device's number of tiles.  Returns {shape: (mean, n,
    simulated mean, combined SE, z, z against the control)}."""
    out = {}
    for (tw, th), mask in tile_shapes(width, height).items():
        got = np.asarray(tile_samples, f64)[mask]
        sim, _ = simulate_stopping(tw, th)
        ctl, _ = simulate_stopping(tw, th, divisor_k=True)
        spread = got.std(ddof=1) if len(got) >= own_spread_from else sim.std(ddof=1)
        se = math.sqrt(spread ** 2 / len(got) + sim.var(ddof=1) / len(sim))
        sec = math.sqrt(spread ** 2 / len(got) + ctl.var(ddof=1) / len(ctl))
        z, zc = (got.mean() - sim.mean()) / se, (got.mean() - ctl.mean()) / sec
        out[(tw, th)] = (got.mean(), len(got), sim.mean(), se, z, zc)
        assert abs(z) <= Z_MAX, f"{what}: tiles of {tw} x {th}: mean count {got.mean()} over {len(got)}, simulated {sim.mean()}, se {se}, z {z}"
        if (tw, th) == (8, 8) and len(got) >= own_spread_from:
            assert abs(zc) > Z_MAX, f"{what}: the control k for k - 1 ({ctl.mean()}) is not rejected: {got.mean()}, z {zc}"
    return out


def frozen_within_tolerance(mean, stderr, tile_samples, width, height):
    """largest stderr_c / (rel_tol |mean_c|) over the pixels of the tiles that froze before the budget (<= 1 is what they were stopped
    by), and the number of such tiles"""
    s = STOP
    t = np.asarray(tile_samples)
    frozen = np.kron(t < s["budget"], np.ones((8, 8), bool))[:height, :width]
    if not frozen.any():
        return 0.0, 0
    lim = s["abs_tol"] + f64(f32(s["rel_tol"])) * np.abs(np.asarray(mean, f64)[frozen])
    return float((np.asarray(stderr, f64)[frozen] / lim).max()), int((t < s["budget"]).sum())


def stop_case(width, height):
    """radiometry_ref's frame Case at the stopping rule's depth and this size: Case.check_means with its own SE cap"""
    lw = law(STOP["D"])
    want = np.tile(lw.closed_forms()[0], (height, width, 1))
    return R.Case(f"sphere-frame-D{STOP['D']}-{width}x{height}-adaptive", R.sphere_scene, "frame", STOP["budget"],
                  R._kw(SEED, STOP["D"], R.SCATTER), want, cam=R.sphere_camera(), size=(width, height))


# ================================================================ D: the robust film
ROBUST = dict(K=8, width=128, height=128, spp=64, depths=(2, 50))
ROBUST_SIM_PIXELS = 20 << 14            # 20 x the frame's pixels: the simulation's SE is 0.22 of the frame's, below the quarter asked for
MEAN, TRIM, GINI = 0, 1, 2              # VK_ROBUST_*


def robust_buckets(lw, rng, pixels, K, spp, chunk=1 << 14):
    """bucket means (pixels, K, 3) in f32 as the header's deposit and resolve step 2 word them: "bucket b = sample % K", "the fixed value
    of a component is trunc(a_c * 2^26)" of the f32 sample, "m_c = ((float)sum_c * 2^-26) / (float)count" """
    assert spp % K == 0
    fixed = np.trunc(lw.table.astype(f32).astype(f64) * 2.0 ** 26).astype(np.int64)
    out = np.empty((pixels, K, 3), f32)
    for p0 in range(0, pixels, chunk):
        p1 = min(pixels, p0 + chunk)
        j = lw.draw_j(rng, (p1 - p0, spp // K, K))          # sample s = i K + b lands in bucket b
        sums = fixed[j].sum(1)
        out[p0:p1] = (sums.astype(f32) * f32(2.0 ** -26)) / f32(spp // K)
    return out


def robust_resolve(m, mode, trim=0):
    """The header's seven resolve steps for bucket means m (pixels, K, 3) of equal, non-zero counts.  Steps 2 to 4 — the luminance, the
    order and the trim — in f32 "unfused, in the order written", because an h that lands on an integer decides a bucket; steps 6 and 7
    in f64.  Returns (rgb (pixels, 3), stderr (pixels, 3), t (pixels,))."""
    m = np.asarray(m, f32)
    P, K, _ = m.shape
    Y = (f32(0.2126) * m[..., 0] + f32(0.7152) * m[..., 1]) + f32(0.0722) * m[..., 2]
    order = np.argsort(Y, axis=1, kind="stable")            # "by Y ascending, ties by bucket index ascending"
    Ys = np.take_along_axis(Y, order, 1)
    ms = np.take_along_axis(m, order[..., None], 1).astype(f64)
    tmax = (K - 2) // 2
    if mode == MEAN:
        t = np.zeros(P, np.int64)
    elif mode == TRIM:
        t = np.full(P, min(trim, tmax), np.int64)
    else:
        num, s = np.zeros(P, f32), np.zeros(P, f32)
        for i in range(1, K + 1):                           # "accumulated ascending from 0"
            num = num + f32(2 * i - K - 1) * Ys[:, i - 1]
            s = s + Ys[:, i - 1]
        ok = (Ys[:, 0] >= 0) & (s > 0)
        G = np.where(ok, num / np.where(ok, f32(K) * s, f32(1)), f32(0)).astype(f32)
        h = (G * f32(K)) * f32(0.5)
        t = np.minimum(np.where(h >= 1, np.floor(h), 0).astype(np.int64), tmax)
    rank = np.arange(K)[None, :]
    kept = (rank >= t[:, None]) & (rank < K - t[:, None])
    q = (K - 2 * t).astype(f64)
    rgb = (ms * kept[..., None]).sum(1) / q[:, None]        # equal counts: the ratio of the integer sums is the mean of the kept means
    e = (((ms - rgb[:, None, :]) ** 2) * kept[..., None]).sum(1)
    return rgb, np.sqrt(e / (q * (q - 1.0))[:, None]), t


@functools.lru_cache(None)
def robust_expected(D, mode, trim=0, pixels=ROBUST_SIM_PIXELS):
    """per channel (mean of rgb / mu, its SE, mean of stderr^2 N / sigma^2, its SE, mean of 2 t / j) over `pixels` pixels of draw()"""
    lw = law(D)
    rgb, se, t = robust_resolve(_robust_sim_buckets(D, pixels), mode, trim)
    b, bse = ratio(rgb / lw.mu)
    v, vse = ratio(se ** 2 * ROBUST["spp"] / lw.var)
    return b, bse, v, vse, float((2.0 * t / ROBUST["K"]).mean())


@functools.lru_cache(2)
def _robust_sim_buckets(D, pixels):
    return robust_buckets(law(D), rng_for(4, D, pixels), pixels, ROBUST["K"], ROBUST["spp"])


def rule_d(rgb, stderr, D, mode, trim, what):
    """the frame's mean of rgb / mu and of stderr^2 N / sigma^2 against the simulation, |z| <= 4 on the combined SE; the simulation's
    own SE at most a quarter of the frame's.  Returns (bias, its SE, z, variance ratio, its SE, z, the simulation's record)."""
    lw = law(D)
    sim = robust_expected(D, mode, trim)
    b, bse = ratio(np.asarray(rgb, f64).reshape(-1, 3) / lw.mu)
    v, vse = ratio(np.asarray(stderr, f64).reshape(-1, 3) ** 2 * ROBUST["spp"] / lw.var)
    assert (sim[1] <= 0.25 * bse * 1.0001).all() and (sim[3] <= 0.25 * vse * 1.0001).all(), f"{what}: simulation SE {sim[1]} {sim[3]} against {bse} {vse}"
    zb = (b - sim[0]) / np.sqrt(bse ** 2 + sim[1] ** 2)
    zv = (v - sim[2]) / np.sqrt(vse ** 2 + sim[3] ** 2)
    assert (np.abs(zb) <= Z_MAX).all(), f"{what}: mean of rgb / mu {b}, simulated {sim[0]}, z {zb}"
    assert (np.abs(zv) <= Z_MAX).all(), f"{what}: mean of stderr^2 N / sigma^2 {v}, simulated {sim[2]}, z {zv}"
    return b, bse, zb, v, vse, zv, sim


# ================================================================ E: temporal accumulation at a fixed camera
TEMPORAL = dict(width=32, height=32, frames=8, windows=(16, 16, 16, 16), D=50, checked=(1, 2, 4, 8))
TEMPORAL_SE_CAP_A = 0.03                 # rule A's cap at 1024 pixels and k = 4; averaging n frames only narrows the spread
TEMPORAL_SE_CAP_VAR = 0.08               # (x - mu)^2 / var of a near-normal mean has spread sqrt(2 + excess): 1.5 / 32 = 0.047; a condition


def frame_seed(frame):
    """the CLI's seeds for successive frames"""
    return SEED + 1 + frame


def rule_e(out_color, out_stderr, n, D, what, control=None):
    """after n frames of N samples each: rule A for out_stderr3 against sigma^2 / (N n), and the pixels' empirical variance of
    out_color (about the known mu) against the same.  control: a wrong frame count n' — sigma^2 / (N n') must be rejected."""
    lw = law(D)
    N = sum(TEMPORAL["windows"])
    var = lw.var / (N * n)
    a = rule_a(out_stderr, var, TEMPORAL_SE_CAP_A, f"{what} out_stderr3 after {n} frames", () if control is None else (n / control,))
    r, se = ratio((np.asarray(out_color, f64).reshape(-1, 3) - lw.mu) ** 2 / var)
    z = (r - 1.0) / se
    assert (se <= TEMPORAL_SE_CAP_VAR).all(), f"{what}: SE {se} of the empirical variance ratio above its cap"
    assert (np.abs(z) <= Z_MAX).all(), f"{what}: the pixels' variance of out_color after {n} frames is {r} of sigma^2 / ({N} * {n}), se {se}, z {z}"
    zc = None
    if control is not None:
        zc = (r - n / control) / se
        assert (np.abs(zc) > Z_MAX).all(), f"{what}: the control n = {control} is not rejected: {r}, se {se}, z {zc}"
    return a, (r, se, z, zc)


MEASURED = """
Measured figures, per channel (r, g, b) unless one number is given.  "draw()": tests/test_estimator_laws.py, numpy alone.  "device": the
public calls on one MI355X, tests/test_gpu_estimator_laws.py; vk_adapt_* (the film) returned vk_progress's figures to the last digit in
every case, as its contract says, and is not listed again.

The law on the per-sample routes (16 x 16 x 1024 samples; emulator and oracle agree sample for sample):
  D = 3:  chi^2 3.1 on 2 degrees of freedom (+0.57 sigma); correlation z: pixel x + 1 +0.48, y + 1 +0.57, sample s + 1 -0.36.
  D = 50: chi^2 61.6 on 32 (+3.70 sigma: inside the 5 asked, and the largest figure of this record); correlation z -1.33, -0.30, -0.15.
  Every sample within 1e-6 of Le a^j up to j = 36; 1.00e-6 to 1.16e-6 for the six samples with j = 37 .. 42 (f32 rounding of j products).

Rule A, R = mean of stderr^2 / (sigma^2 / N), its SE, z; control z for the divisor k [and equally weighted windows]:
  plan      D   draw(): R, SE, z                               device: R, SE, z                                   device controls
  equal     3   1.031 1.041 1.041  0.0265  +1.2 +1.5 +1.5      1.006 0.983 0.964  0.0245  +0.2 -0.7 -1.5          +10.3 +9.5 +8.8
  equal     50  0.976 0.973 0.962  0.0252  -0.9 -1.1 -1.5      1.006 0.986 0.965  0.0246  +0.3 -0.6 -1.4          +10.3 +9.6 +8.8
  unequal   3   1.014 1.018 1.018  0.0258  +0.6 +0.7 +0.7      0.985 0.972 0.964  0.0243  -0.6 -1.1 -1.5          +9.3 +9.2 +9.1 [-28.7 -30.5 -31.6]
  unequal   50  0.972 0.971 0.979  0.0245  -1.2 -1.2 -0.8      0.985 0.971 0.956  0.0242  -0.6 -1.2 -1.9          +9.3 +9.2 +8.9 [-28.7 -30.7 -32.3]
  k8        3   0.994 0.995 0.997  0.0082  -0.7 -0.6 -0.4      0.995 0.991 0.989  0.0082  -0.6 -1.1 -1.4          +14.7 +14.2 +13.9
  k8        50  1.028 1.028 1.017  0.0085  +3.3 +3.3 +2.1      0.995 0.991 0.991  0.0082  -0.6 -1.1 -1.1          +14.7 +14.2 +14.2
  k2        3   1.044 1.033 1.022  0.0467  +1.0 +0.7 +0.5      1.049 1.046 1.034  0.0443  +1.1 +1.0 +0.8          +12.4 +12.4 +12.4
  k2        50  0.991 1.013 1.028  0.0476  -0.2 +0.3 +0.6      1.048 1.034 0.990  0.0450  +1.1 +0.8 -0.2          +12.4 +12.0 +10.9
  equal64   3   0.987 0.992 0.999  0.0126  -1.1 -0.6 -0.1      1.003 0.999 0.995  0.0127  +0.3 -0.1 -0.4          +20.2 +19.7 +19.3
  equal64   50  1.027 1.021 1.010  0.0130  +2.0 +1.6 +0.8      1.004 1.002 1.002  0.0126  +0.3 +0.2 +0.2          +20.2 +20.0 +20.1
  k8_128    3   1.008 1.006 1.005  0.0042  +1.8 +1.5 +1.2      0.999 0.998 0.997  0.0041  -0.3 -0.6 -0.8          +29.9 +29.6 +29.4
  k8_128    50  1.000 1.000 1.000  0.0042  -0.0 -0.0 -0.0      0.999 0.997 0.995  0.0041  -0.3 -0.8 -1.3          +29.9 +29.5 +29.1
  (SE: the largest channel.  The caps 0.03 / 0.01 / 0.05 leave 12 % / 15 % / 5 % of room.)  Equally weighted window means on draw(),
  2^14 pixels: 1.723 1.719 1.716 +- 0.013 of sigma^2 / N against the 1.7083 of control_equal_weights().

Rule B, the share of pixels within 2 stderr, 2^18 pixels of draw() (expected / control):
  k = 4 (equal):   D = 3 0.8607 0.8608 0.8607 / 0.8187 0.8207 0.8186;  D = 50 0.8591 0.8599 0.8611 / 0.8171 0.8174 0.8194
  k = 4 (unequal): D = 3 0.8609 0.8616 0.8614 / 0.8187 0.8193 0.8193;  D = 50 0.8599 0.8606 0.8611 / 0.8173 0.8183 0.8192
  k = 8:           D = 3 0.9138 0.9143 0.9148 / 0.8960 0.8967 0.8967;  D = 50 0.9134 0.9140 0.9149 / 0.8952 0.8958 0.8969
  k = 2:           D = 3 0.7217 0.7399 0.6877 / 0.6481 0.5655 0.5682;  D = 50 0.7188 0.7000 0.7020 / 0.6502 0.6040 0.6059
  (a normal mean would give 0.861, 0.918 and 0.705: only k = 2 at D = 3 is visibly not normal.)
  control_power_b: 3.3 to 3.5 (equal, unequal: 1024 pixels), 3.7 to 3.8 (k8: 4096), 4.6 to 11.2 (k2), 6.6 to 7.0 (equal64), 7.2 to 7.4 (k8_128).
  device, z against the expected share / against the control (asked of the channels marked *):
  equal     D = 3 -0.3 +0.6 +0.3 / 3.2 3.9 3.8          D = 50 -0.2 +0.7 +1.3 / 3.3 4.1 4.6
  unequal   D = 3 -1.6 -2.0 +0.3 / 2.1 1.7 3.7          D = 50 -1.1 -0.0 +0.4 / 2.5 3.5 3.8
  k8        D = 3 +0.7 -1.5 -1.0 / 4.3 2.3 2.8          D = 50 +0.5 -0.0 +0.5 / 4.2 3.7 4.2
  k2        D = 3 +0.5 +0.4 -0.1 / 5.4 11.6* 7.6*       D = 50 -0.0 -0.2 -1.6 / 4.6 6.1* 4.8*
  equal64   D = 3 +1.2 +0.0 +0.7 / 8.0* 6.7* 7.6*       D = 50 +1.8 +0.2 +0.3 / 8.5* 7.2* 7.1*
  k8_128    D = 3 -0.2 -0.2 -0.4 / 7.0* 7.0* 7.0*       D = 50 -0.2 +0.6 +0.2 / 7.2* 7.9* 7.6*
  draw(), frames of the same sizes: |z| <= 2.2 against the expected share; the asked controls rejected by 5.4 to 12.1.

Rule C, simulation of 2048 tiles per shape (mean count +- spread; the control k for k - 1; frozen mean / mu - 1 in units of 1e-4 +- SE):
  8 x 8: 182.9 +- 23.7; 156.6;  +2.3 +1.0 +0.1 +- 2.9 2.0 1.0       4 x 8: 168.3 +- 26.4; 140.9;  +8.5 +6.4 +2.9 +- 4.3 2.9 1.5
  8 x 4: 167.9 +- 26.4; 139.2;  -5.6 -2.3 -0.6 +- 4.3 3.0 1.5       4 x 4: 150.7 +- 29.4; 117.9;  -4.9 -3.2 -1.4 +- 6.4 4.3 2.1
  no stopping bias beyond 2.2 SE in any shape.  64 fresh tiles of draw(): 185.0, z +0.64, control z +8.7.
  device, 64 x 64: 179.5 over 64 tiles, combined SE 2.86, z -1.19, control z +7.97; all 64 tiles froze, worst stderr / tolerance 0.9995;
    frozen frame / closed form 1.0019 1.0009 1.0000, SE 0.0016 0.0011 0.0006, z +1.2 +0.8 +0.1.
  device, 44 x 36: 8 x 8 184.0 over 20 (z +0.27, control z +6.9); 4 x 8 168.0 over 4 (z -0.02); 8 x 4 172.8 over 5 (z +0.41); 4 x 4 160 (one
    tile, z +0.32); 30 tiles froze, worst stderr / tolerance 0.9975; frozen frame / closed form 1.0056 1.0030 1.0008, SE 0.0026 0.0018
    0.0009, z +2.1 +1.7 +0.9.

Rule D, K = 8, 128 x 128 x 64 spp; simulation of 327 680 pixels (rgb / mu +- SE; stderr^2 N / sigma^2; mean 2 t / j):
  D = 2  TRIM 1: 0.9774 +- 0.0004; 0.7051; 0.25         GINI: 0.9782 +- 0.0004; 0.7533; 0.185        (the three channels are proportional)
  D = 50 TRIM 1: 0.9831 0.9940 1.0006 +- 0.0003 0.0002 0.0001; 0.727 0.657 0.723; 0.25
         GINI:   0.9993 0.9997 0.9999 +- 0.0003 0.0002 0.0001; 0.993 0.992 0.993; 0.0024
  device, MEAN: stderr^2 N / sigma^2 D = 2 1.0008 +- 0.0041 (z +0.2, divisor K: z +30.5); D = 50 1.0015 1.0021 1.0018 +- 0.0041 (z +0.4
    +0.5 +0.5, control +30.8 +31.4 +31.4); rgb / mu D = 2 1.0015 +- 0.0017; D = 50 1.0012 1.0005 1.0000 +- 0.0014 0.0009 0.0005.
  device, TRIM 1: D = 2 rgb / mu 0.9788 +- 0.0018 (z +0.76; against the unbiased value -11.7), stderr^2 0.7007 +- 0.0037 (z -1.19);
    D = 50 0.9838 0.9942 1.0006 (z +0.5 +0.3 +0.0), stderr^2 0.7231 0.6558 0.7218 (z -1.0 -0.4 -0.3).
  device, GINI: D = 2 0.9800 +- 0.0018 (z +0.96; against the unbiased value -11.1), stderr^2 0.7517 (z -0.43);
    D = 50 1.0005 1.0002 1.0000 (z +0.9 +0.6 +0.1), stderr^2 0.9963 0.9958 0.9960 (z +0.8 +0.9 +0.8).
  every bias within the trimmed share 2 t / j.  The host build of the resolve (emu_robust_ffi, 64 x 64 pixels of draw()): MEAN R 1.0017
    (D = 2), 1.0016 1.0041 1.0053 (D = 50), SE 0.0081, control z +15.6 to +16.3; TRIM and GINI |z| <= 1.0 against the simulation.

Rule E, 32 x 32, 8 frames of 64 samples (R of out_stderr3, its z; the pixels' spread of out_color, its z):
  draw() D = 3:  n = 1 1.047 1.024 1.002 (+1.8 +0.9 +0.1), 0.933 0.925 0.928 (-1.7 -1.9 -1.8);  n = 4 1.013 1.010 1.007, 0.876 0.889 0.927
                 (-3.3 -2.8 -1.8), control z -11.9 -11.4 -9.9;  n = 8 1.005 1.006 1.006, 0.959 0.972 0.993 (-1.0 -0.6 -0.2)
  draw() D = 50: n = 1 0.986 0.973 0.975, 1.015 0.986 0.954;  n = 4 1.023 1.012 1.003, 0.971 0.998 0.995, control z -8.5 -7.5 -7.5;  n = 8 1.013
                 1.006 1.003 (+1.4 +0.7 +0.3), 0.948 0.964 0.965 (-1.2 -0.8 -0.8)
  SE of the spread statistic 0.038 to 0.049.  Its z is left-skewed (a frame without a far pixel has a small mean AND a small SE): over
  400 single frames of draw() per depth, mean -0.03, spread 1.01, smallest -3.84, largest +2.73.  The frame first drawn for the D = 3
  self-test (generator key 8) gave -4.04 in blue at n = 1; the self-test now draws key 9.
  device D = 3:  n = 1 1.020 1.024 1.029 (+0.8 +1.0 +1.1), 1.014 1.010 0.990 (+0.3 +0.2 -0.2);  n = 2 1.001 1.005 1.012, 1.012 1.005 0.987;
                 n = 4 0.991 0.995 1.000 (-0.7 -0.4 +0.0), 1.050 1.074 1.078 (+1.0 +1.4 +1.5), control z -27.2 -27.0 -26.9 (out_stderr3) and
                 -5.6 -5.0 -5.1 (spread);  n = 8 0.997 1.000 1.002 (-0.4 -0.0 +0.2), 1.019 1.042 1.048 (+0.4 +0.9 +1.0)
  device D = 50: n = 1 1.020 1.021 1.010 (+0.8 +0.8 +0.4), 1.014 1.005 0.986;  n = 2 1.002 1.008 1.005, 1.011 1.006 1.015;  n = 4 0.991 0.993
                 0.987 (-0.7 -0.6 -1.0), 1.048 1.069 1.076 (+1.0 +1.4 +1.6), control z -27.1 -27.4 -28.1 and -5.7 -5.3 -5.4;  n = 8 0.997 0.997
                 0.992 (-0.4 -0.3 -0.9), 1.015 1.018 1.009 (+0.3 +0.4 +0.2)
  SE of the device's out_stderr3 ratio 0.026 / 0.018 / 0.013 / 0.009 at n = 1 / 2 / 4 / 8; every pixel's history length n to f32 rounding.

Time: the GPU module 11 s on one MI355X (30 tests; the coverage simulation of a depth, 2 s, is the largest piece), the CPU module 30 s.
"""
