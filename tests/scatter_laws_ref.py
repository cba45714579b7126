"""Closed-form scattering and light-sampling laws: what ONE bounce draws.  TESTS ONLY; shared by tests/test_scatter_laws.py (the shade
emulator) and tests/test_gpu_scatter_laws.py (vk_shade_hits and a path batch on the device).

Everything here is plain f64 numpy written from the reference's own lines (material.rs, util.rs, hittable.rs, main.rs; cited beside
each law) and shares nothing with the library's restatement of them: no import of the oracle, of an emulator or of another *_ref.py, no
formula taken from vk_trace.h.  From vecchio_amd only the ffi constants, the record dtypes and make_path_states / make_rays.  The RNG
stream is not under test: every expected value is a property of the DISTRIBUTION a law draws from, or a per-sample identity between the
outputs of one item.

A case is N hand-made (ray, hit, state) items that share p, normal, front, material, incoming direction (not unit length) and time
0.37; make_path_states(N, seed) gives each item a stream of its own.  One bounce of vk_shade_hits turns them into N draws of the law.

The rule (Report):
  * a mean over n samples:  |mean - want| <= 4 SE, SE = s / sqrt(n) from the samples;
  * a share k / n:          |k / n - p| <= 4 sqrt(p (1 - p) / n), SE from the closed form;
  * 4 is radiometry_ref.Z_MAX's value.  There is no SE cap (many expectations are 0); non-vacuity comes from the power controls: every
    family of statistics names a plausible wrong law, and the same data must reject it by |z| > 8;
  * N = 65 536 items per case: a condition, not a measurement;
  * seeds are fixed (SEEDS below).  A statistic that fails is not cured by another seed: the case is run once more at 4 N with a second
    seed; a real deviation doubles its z, a fluctuation does not ("Closed-form scattering laws", records the outcomes).

Deterministic tolerances (derived, not measured from the code under test):
  * identities on unit-scale f32 outputs (|d - normal| = 1, |d| = 1, mirror and Snell directions, |d - z w| = 1 - z^2, a point in its
    rect's plane): 2e-6 absolute = 32 units of 2^-24, for at most a dozen rounded f32 operations and one sine / cosine pair;
  * the weight identity thr = albedo spdf(d) / pdf(d): 1e-5 relative, for about 40 rounded f32 operations on positive, well-conditioned
    terms; the f64 side starts from the RETURNED f32 direction, so it carries no input error;
  * exact values ((1, 0, 0), 0, NaN-ness, a copied field) are compared exactly, 2 albedo and 4 albedo to 4 ulp.

Stability: a sample is out of the weight identity only when f32 and f64 could place its direction on opposite sides of a decision:
within 1e-4 (of the rect's size) of a rect edge, a grazing margin sqrt(disc) / (|d| r) < 1e-3 on a sphere light, either cosine below
1e-3 (a cosine that is exactly 0 in f64 is exactly 0 in f32 too — the default draw (1, 0, 0) against a normal without an x component —
and stays in).  At most 1 % of a case's samples may be excluded, asserted per case."""
import math

import numpy as np

from descs import Desc
from vecchio_amd import ffi
from vecchio_amd.scene import HIT_DTYPE, PATH_STATE_DTYPE, RAY_DTYPE, make_path_states, make_rays  # noqa: F401

f64, f32 = np.float64, np.float32
Z_MAX = 4.0                        # radiometry_ref.Z_MAX's value
Z_CONTROL = 8.0
N = 65536
TOL_UNIT = 2e-6                    # 32 * 2^-24
TOL_WEIGHT = 1e-5
ULP4 = 4.0 * 2.0 ** -23            # 4 ulp, relative
EDGE_MIN, GRAZE_MIN, COS_MIN = 1e-4, 1e-3, 1e-3
MAX_EXCLUDED = 0.01
TMIN = 0.001                       # main.rs:130, hittable.rs:105, 272
TIME = 0.37
PDF, SCATTER = ffi.VK_INTEGRATOR_PDF, ffi.VK_INTEGRATOR_SCATTER
INTEG_NAME = {PDF: "pdf", SCATTER: "scatter"}
SCATTERED, ENDED, MISS = ffi.VK_SHADE_SCATTERED, ffi.VK_SHADE_ENDED, ffi.VK_SHADE_MISS


def unit(v):
    v = np.asarray(v, f64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def dot(a, b):
    return (np.asarray(a, f64) * np.asarray(b, f64)).sum(-1)


def tangents(nh):
    """two unit vectors that complete nh to an orthonormal frame.  WHICH two is free: every law below is symmetric about its axis, so
    the frame's handedness and azimuth are not pinned (and cannot be)"""
    a = np.array([0.0, 1.0, 0.0]) if abs(nh[0]) > 0.9 else np.array([1.0, 0.0, 0.0])
    t1 = unit(np.cross(nh, a))
    return t1, np.cross(nh, t1)


# ================================================================ closed forms
def cap_share(fuzz, cosine):
    """share of reflected + fuzz * B, B uniform in the unit ball (util.rs:31-39), that ends at or below the surface, for a mirror
    direction whose cosine against the unit normal is `cosine` < fuzz: the cap of a ball of radius f cut at depth cosine below its
    centre has height a = f - cosine and volume pi a^2 (3 f - a) / 3, over 4 pi f^3 / 3"""
    a = fuzz - cosine
    return a * a * (3.0 * fuzz - a) / (4.0 * fuzz ** 3)


def cap_share_surface(fuzz, cosine):
    """the same share were the fuzz drawn ON the sphere (Archimedes: the area of a cap is proportional to its height): the control"""
    return (fuzz - cosine) / (2.0 * fuzz)


def schlick(cosine, ref_idx):
    """util.rs:25-29"""
    r0 = ((1.0 - ref_idx) / (1.0 + ref_idx)) ** 2
    return r0 + (1.0 - r0) * (1.0 - cosine) ** 5


def reflect(v, n):
    """util.rs:14-16"""
    return v - n * (2.0 * dot(v, n))


def refract(uv, n, eta):
    """util.rs:18-23"""
    cos_theta = -dot(uv, n)
    par = (uv + n * cos_theta) * eta
    return par - n * math.sqrt(1.0 - dot(par, par))


BALL_X2, BALL_R3 = 1.0 / 5.0, 1.0 / 2.0      # E[x^2] and E[|d|^3] of the uniform unit ball: int r^2 r^2 dr / int r^2 dr / 3, 3 int r^5 dr
SPHERE_X2 = 1.0 / 3.0                        # E[x^2] on the unit sphere's surface


def cone_moments(cm):
    """z uniform on [cm, 1] (hittable.rs:127): (E z, Var z, E[1 - z^2], E sqrt(1 - z^2)); the third is the length random_to_sphere
    gives the part of the direction across the axis (hittable.rs:130-131), the last what the textbook cone would give it"""
    ez, var = (1.0 + cm) / 2.0, (1.0 - cm) ** 2 / 12.0
    e_lin = 1.0 - (1.0 + cm + cm * cm) / 3.0
    prim = lambda z: 0.5 * (z * math.sqrt(1.0 - z * z) + math.asin(z))
    return ez, var, e_lin, (prim(1.0) - prim(cm)) / (1.0 - cm)


# ---------------------------------------------------------------- what `lights` holds, as plain numbers
class RectL:
    """Rect::hit, pdf_value, random: hittable.rs:230-256, 271-292"""

    def __init__(self, c0, c1, d0, d1, k, axes):
        self.c0, self.c1, self.d0, self.d1, self.k, self.axes = float(c0), float(c1), float(d0), float(d1), float(k), tuple(axes)
        self.area = (self.c1 - self.c0) * (self.d1 - self.d0)

    def add(self, d):
        return d.rect(self.c0, self.c1, self.d0, self.d1, self.k, self.axes, d.light(0, 0, 0))

    def pdf(self, o, v):
        """(pdf_value(o, v), unstable) for directions v (n, 3): t^2 |v|^2 / (|v . n| / |v| * area) where the ray meets the rect within
        [0.001, inf), else 0; every comparison as Rect::hit makes it (a NaN passes)"""
        a0, a1, a2 = self.axes
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (self.k - o[a2]) / v[:, a2]
            a, b = o[a0] + t * v[:, a0], o[a1] + t * v[:, a1]
            miss = (t < TMIN) | (t > np.inf) | (a < self.c0) | (a > self.c1) | (b < self.d0) | (b > self.d1)
            length = np.sqrt(dot(v, v))
            cosine = np.abs(v[:, a2]) / length
            value = np.where(miss, 0.0, t * t * length * length / (cosine * self.area))
            sa, sb = self.c1 - self.c0, self.d1 - self.d0
            near_a = (np.minimum(np.abs(a - self.c0), np.abs(a - self.c1)) < EDGE_MIN * sa) & (b > self.d0 - EDGE_MIN * sb) & \
                (b < self.d1 + EDGE_MIN * sb)
            near_b = (np.minimum(np.abs(b - self.d0), np.abs(b - self.d1)) < EDGE_MIN * sb) & (a > self.c0 - EDGE_MIN * sa) & \
                (a < self.c1 + EDGE_MIN * sa)
            unstable = (t >= TMIN) & (near_a | near_b | (~miss & (cosine < COS_MIN)))
        return value, unstable

    def inside(self, q, tol):
        a0, a1, a2 = self.axes
        return ((np.abs(q[:, a2] - self.k) <= tol) & (q[:, a0] >= self.c0 - tol) & (q[:, a0] <= self.c1 + tol)
                & (q[:, a1] >= self.d0 - tol) & (q[:, a1] <= self.d1 + tol))


class BoxL:
    """Boxy: six sides, three of them FlipFace'd (hittable.rs:321-359); pdf_value and random are the side list's (:371-377), which is
    Vec's (:420-433): the mean of the sides' values, a side chosen evenly.  A FlipFace'd side forwards neither (:299-311) and falls back
    to the trait defaults (:36-41)"""

    def __init__(self, p0, p1):
        self.p0, self.p1 = tuple(float(x) for x in p0), tuple(float(x) for x in p1)
        (x0, y0, z0), (x1, y1, z1) = self.p0, self.p1
        self.plain = [RectL(x0, x1, y0, y1, z1, (0, 1, 2)), RectL(x0, x1, z0, z1, y1, (0, 2, 1)), RectL(y0, y1, z0, z1, x1, (1, 2, 0))]

    def add(self, d):
        return d.boxy(self.p0, self.p1, d.light(0, 0, 0))

    def pdf(self, o, v):
        total, unstable = np.zeros(len(v)), np.zeros(len(v), bool)
        for side in self.plain:
            value, u = side.pdf(o, v)
            total, unstable = total + value / 6.0, unstable | u
        return total, unstable


class DefaultL:
    """an entry that forwards neither pdf_value nor random — a FlipFace (hittable.rs:299-311), a MovingSphere (:186-197 implements
    hit and bounding_box only) — and so answers 0 and (1, 0, 0) (hittable.rs:36-41)"""

    def __init__(self, add):
        self.add = add

    def pdf(self, o, v):
        return np.zeros(len(v)), np.zeros(len(v), bool)


class SphereL:
    """Sphere::hit, pdf_value, random and random_to_sphere: hittable.rs:65-95, 104-134"""

    def __init__(self, center, radius):
        self.center, self.radius = np.asarray(center, f64), float(radius)

    def add(self, d):
        return d.sphere(tuple(self.center), self.radius, d.light(0, 0, 0))

    def cos_max(self, o):
        return math.sqrt(1.0 - self.radius ** 2 / dot(self.center - o, self.center - o))

    def pdf(self, o, v):
        oc = o - self.center
        a, half_b, c = dot(v, v), dot(v, oc), dot(oc, oc) - self.radius ** 2
        disc = half_b * half_b - a * c
        root = np.sqrt(np.maximum(disc, 0.0))
        t1, t2 = (-half_b - root) / a, (-half_b + root) / a
        hit = (disc > 0.0) & ((TMIN < t1) | (TMIN < t2))
        value = np.where(hit, 1.0 / (2.0 * math.pi * (1.0 - self.cos_max(o))), 0.0)
        # beside the margin, the discriminant's own cancellation (geometry_ref.CANCEL_MIN's reasoning: half_b^2 - a c is a difference
        # of terms of size a |oc|^2 that carry a few ulp each; below 16 ulp of them its f32 sign is rounding)
        cancelled = np.abs(disc) < 1e-6 * a * (dot(oc, oc) + self.radius ** 2)
        return value, (np.sqrt(np.abs(disc)) / (np.sqrt(a) * self.radius) < GRAZE_MIN) | cancelled


def lights_pdf(lights, o, v):
    """Vec::pdf_value over the entries of `lights` (hittable.rs:420-427; main.rs:139, 169): (value, unstable)"""
    total, unstable = np.zeros(len(v)), np.zeros(len(v), bool)
    for l in lights:
        value, u = l.pdf(o, v)
        total, unstable = total + value / len(lights), unstable | u
    return total, unstable


# ================================================================ the rule
class Report:
    """collects the statistics, identities and controls of one case; finish() asserts all of them at once, so that a failing run names
    every statistic that failed"""

    def __init__(self, name):
        self.name, self.stats, self.controls, self.idents, self.failures, self.excluded = name, [], [], {}, [], 0.0

    def _stat(self, what, got, want, se, control):
        z = 0.0 if got == want else (got - want) / se if se > 0 else math.inf
        self.stats.append((what, got, want, se, z))
        if not abs(got - want) <= Z_MAX * se:
            self.failures.append(f"{what}: {got:.6g}, want {want:.6g}, se {se:.3g}, z {z:.2f}")
        if control is not None:
            zc = (got - control) / se if se > 0 else math.inf
            self.controls.append((what, control, zc))
            if not abs(zc) > Z_CONTROL:
                self.failures.append(f"{what}: the control {control:.6g} is not rejected, z {zc:.2f}")

    def mean(self, what, x, want, control=None):
        x = np.asarray(x, f64)
        if len(x) < 2:
            self.failures.append(f"{what}: {len(x)} samples")
            return
        self._stat(what, float(x.mean()), float(want), float(x.std(ddof=1)) / math.sqrt(len(x)), control)

    def share(self, what, k, n, p, control=None):
        k = int(np.count_nonzero(k)) if isinstance(k, np.ndarray) else int(k)
        self._stat(what, k / n, float(p), math.sqrt(p * (1.0 - p) / n), control)

    def ident(self, what, deviation, tol):
        dev = np.abs(np.asarray(deviation, f64))
        worst = float(dev.max()) if dev.size else 0.0
        self.idents[what] = max(self.idents.get(what, 0.0), worst)
        if not worst <= tol:                      # (a NaN fails)
            self.failures.append(f"{what}: deviation {worst:.3g} above {tol:.3g} ({int((~(dev <= tol)).sum())} of {dev.size})")

    def exact(self, what, ok):
        ok = np.asarray(ok)
        if not ok.all():
            self.failures.append(f"{what}: {int((~ok).sum())} of {ok.size} items")

    def exclude(self, unstable):
        self.excluded = max(self.excluded, float(np.count_nonzero(unstable)) / max(1, len(unstable)))
        if self.excluded > MAX_EXCLUDED:
            self.failures.append(f"{self.excluded:.4f} of the samples excluded from the weight identity")

    def worst_z(self):
        return max((abs(s[4]) for s in self.stats), default=0.0)

    def weakest_control(self):
        return min((abs(c[2]) for c in self.controls), default=math.inf)

    def summary(self):
        ids = ", ".join(f"{k} {v:.2e}" for k, v in self.idents.items())
        return (f"{self.name}: {len(self.stats)} statistics, worst |z| {self.worst_z():.2f}; {len(self.controls)} controls, weakest |z| "
                f"{self.weakest_control():.1f}; excluded {self.excluded:.5f}; {ids}")

    def finish(self):
        assert not self.failures, f"{self.name}:\n  " + "\n  ".join(self.failures)
        return self


# ================================================================ one bounce's outputs as f64
class Out:
    def __init__(self, out, rays, hits, states, has_lobe=True):
        self.has_lobe = has_lobe           # (a path batch reports no lobe)
        assert len(out) == len(rays) == len(hits) == len(states)
        for a in (rays["direction"], rays["time"], hits["p"], hits["normal"], hits["front"], hits["material"]):
            assert (a == a[0]).all(), "the items of a case share their ray and hit"
        self.n = len(out)
        self.p, self.normal = hits["p"][0].astype(f64), hits["normal"][0].astype(f64)
        self.front, self.d_in, self.time_in = bool(hits["front"][0]), rays["direction"][0].astype(f64), rays["time"][0]
        self.p32, self.states, self.out = hits["p"][0], states, out
        self.d, self.time = out["next"]["direction"].astype(f64), out["next"]["time"]
        self.thr, self.acc = out["state"]["thr"].astype(f64), out["state"]["acc"].astype(f64)
        self.thr32, self.status, self.lobe = out["state"]["thr"], out["status"], out["lobe"]
        self.all = np.ones(self.n, bool)


def check_copied(R, X):
    """what a bounce must leave alone: the stream's identity; depth + 1 (main.rs:136, 146)"""
    st, o = X.states, X.out["state"]
    R.exact("seed, pixel, sample copied", (o["seed"] == st["seed"]) & (o["pixel"] == st["pixel"]) & (o["sample"] == st["sample"]))
    live = X.status == SCATTERED
    R.exact("depth + 1", o["depth"][live] == st["depth"][live] + 1)
    R.exact("_pad 0", X.out["_pad"] == 0)


def check_scattered(R, X, sel, lobe, time, what=""):
    """a live item: the next ray starts at the hit's p with tmax = inf and the law's time; nothing was emitted"""
    nx = X.out["next"][sel]
    R.exact(f"{what}status SCATTERED", X.status[sel] == SCATTERED)
    if X.has_lobe:
        R.exact(f"{what}lobe", X.lobe[sel] == lobe)
    R.exact(f"{what}origin = p", nx["origin"].view(np.uint32) == X.p32.view(np.uint32))
    R.exact(f"{what}tmax = inf", np.isposinf(nx["tmax"]))
    R.exact(f"{what}time", nx["time"] == f32(time))
    R.exact(f"{what}acc = 0", X.out["state"]["acc"][sel] == 0)


def check_ended(R, X, sel, what=""):
    R.exact(f"{what}ENDED: next zeros", X.out["next"][sel].view(np.uint32) == 0)


# ================================================================ the laws
def law_lambertian_scatter(R, X, albedo):
    """Lambertian::scatter, material.rs:85-90, with Lambertian::random, :51-58: d = normal + U, U uniform ON the unit sphere (z uniform,
    azimuth uniform), not normalised; attenuation the albedo; r.time kept.  Control: U uniform IN the ball (random_in_unit_sphere)."""
    n = X.normal
    check_scattered(R, X, X.all, ffi.VK_MAT_LAMBERTIAN, X.time_in)
    u = X.d - n
    R.ident("|d - normal| = 1", np.sqrt(dot(u, u)) - 1.0, TOL_UNIT)
    for i in range(3):
        R.mean(f"E[d].{'xyz'[i]}", X.d[:, i], n[i])
        for j in range(i, 3):
            R.mean(f"Cov {'xyz'[i]}{'xyz'[j]}", u[:, i] * u[:, j], SPHERE_X2 if i == j else 0.0, BALL_X2 if i == j else None)
    if abs(math.sqrt(dot(n, n)) - 1.0) < 1e-6:
        # |n + U|^2 = 2 + 2 z and (n + U) . n = 1 + z for z = U . n, so cos^2 = (1 + z) / 2: uniform on [0, 1]
        c2 = dot(unit(X.d), n) ** 2
        R.mean("cos^2: mean", c2, 1.0 / 2.0)
        R.mean("cos^2: second moment", c2 * c2, 1.0 / 3.0)
    R.exact("thr = albedo", X.thr32 == f32(albedo))


def law_metal(R, X, sel, albedo, fuzz, integrator, what=""):
    """Metal, material.rs:118-141: reflected = reflect(unit(v), n) (util.rs:14-16), d = reflected + fuzz * B, B uniform IN the unit ball
    (util.rs:31-39).  scatter (:118-132) keeps r.time and absorbs unless d . n > 0; scatter_with_pdf (:134-141) makes a specular ray
    with Ray::new — time 0 — and has no such test, so the PDF integrator (main.rs:134-137) follows it below the surface too.
    Controls: B ON the sphere (the share a / 2f, the covariance f^2 / 3)."""
    n = X.normal
    mirror = reflect(unit(X.d_in), n)
    cos_r = float(dot(mirror, n))
    d = X.d[sel]
    count = int(sel.sum())
    if fuzz == 0.0:
        check_scattered(R, X, sel, ffi.VK_MAT_METAL, 0.0 if integrator == PDF else X.time_in, what)
        R.ident(f"{what}d = reflect(unit(v), n)", np.abs(d - mirror).max(-1, initial=0.0), TOL_UNIT)
        R.exact(f"{what}thr = albedo", X.thr32[sel] == f32(albedo))
        return
    cap = cap_share(fuzz, cos_r)
    t1, t2 = tangents(n)
    if integrator == SCATTER:
        ended = sel & (X.status == ENDED)
        live = sel & ~ended
        R.share(f"{what}ENDED share", ended, count, cap, cap_share_surface(fuzz, cos_r))
        check_ended(R, X, ended, what)
        check_scattered(R, X, live, ffi.VK_MAT_METAL, X.time_in, what)
        R.exact(f"{what}survivors have d . n > 0", dot(X.d[live], n) > 0)
        # the cut is across n: what survives keeps the ball's symmetry about the mirror direction's tangential part
        R.mean(f"{what}E[d . t1 | live]", dot(X.d[live], t1), dot(mirror, t1))
        R.mean(f"{what}E[d . t2 | live]", dot(X.d[live], t2), dot(mirror, t2))
        R.exact(f"{what}thr = albedo", X.thr32[live] == f32(albedo))
        R.exact(f"{what}|d - reflected| < fuzz", np.sqrt(dot(X.d[live] - mirror, X.d[live] - mirror)) < fuzz + TOL_UNIT)
        return
    check_scattered(R, X, sel, ffi.VK_MAT_METAL, 0.0, what)
    u = d - mirror
    R.exact(f"{what}|d - reflected| < fuzz", np.sqrt(dot(u, u)) < fuzz + TOL_UNIT)
    R.share(f"{what}share below the surface", dot(d, n) <= 0, count, cap, cap_share_surface(fuzz, cos_r))
    for i in range(3):
        R.mean(f"{what}E[d].{'xyz'[i]}", d[:, i], mirror[i])
        for j in range(i, 3):
            R.mean(f"{what}Cov {'xyz'[i]}{'xyz'[j]}", u[:, i] * u[:, j], fuzz ** 2 * BALL_X2 if i == j else 0.0,
                   fuzz ** 2 * SPHERE_X2 if i == j else None)
    R.exact(f"{what}thr = albedo", X.thr32[sel] == f32(albedo))


def law_dielectric(R, X, ref_idx, control):
    """Dielectric, material.rs:150-206 (both routes alike): etai_over_etat = 1 / ref_idx on the front face, ref_idx on the back;
    cos = min(-unit(v) . n, 1); total internal reflection where etai_over_etat * sin > 1, else reflected with probability
    schlick(cos, etai_over_etat) (util.rs:25-29: the INCIDENT cosine on either side), else refract (util.rs:18-23: Snell's law);
    attenuation white, r.time kept.  control: 'r0' (Schlick without its angular term), 'transmitted' (the angular term on the
    transmitted angle's cosine, as some texts have it for the denser side) or None where neither differs from the law by more than a
    fluctuation: at cos 0.9 the term is 0.96 * 10^-5."""
    n, uv = X.normal, unit(X.d_in)
    eta = 1.0 / ref_idx if X.front else ref_idx
    cos = min(float(-dot(uv, n)), 1.0)
    sin = math.sqrt(1.0 - cos * cos)
    check_scattered(R, X, X.all, ffi.VK_MAT_DIELECTRIC, X.time_in)
    R.exact("thr unchanged", X.thr32 == X.states["thr"])
    mirror = reflect(uv, n)
    to_mirror = np.abs(X.d - mirror).max(-1)
    if eta * sin > 1.0:
        R.ident("d = reflect(unit(v), n)", to_mirror, TOL_UNIT)
        return
    bent = refract(uv, n, eta)
    assert abs(math.sqrt(1.0 - dot(bent, n) ** 2) - eta * sin) < 1e-12          # Snell: sin' = eta sin
    to_bent = np.abs(X.d - bent).max(-1)
    reflected = to_mirror < to_bent
    R.ident("d = reflect or refract", np.minimum(to_mirror, to_bent), TOL_UNIT)
    r0 = ((1.0 - eta) / (1.0 + eta)) ** 2
    wrong = {None: None, "r0": r0, "transmitted": r0 + (1.0 - r0) * (1.0 - abs(float(dot(bent, n)))) ** 5}[control]
    R.share("share reflected", reflected, X.n, schlick(cos, eta), wrong)


def law_isotropic_scatter(R, X, albedo):
    """Isotropic::scatter, material.rs:441-446: d = random_in_unit_sphere() (util.rs:31-39: uniform IN the ball, by rejection), not
    normalised; attenuation the albedo; r.time kept.  Control: uniform ON the sphere."""
    check_scattered(R, X, X.all, ffi.VK_MAT_ISOTROPIC, X.time_in)
    r = np.sqrt(dot(X.d, X.d))
    R.exact("|d| < 1", r < 1.0)
    for i in range(3):
        R.mean(f"E[d].{'xyz'[i]}", X.d[:, i], 0.0)
        R.mean(f"E[{'xyz'[i]}^2]", X.d[:, i] ** 2, BALL_X2, SPHERE_X2)
    R.mean("E[|d|^3]", r ** 3, BALL_R3, 1.0)
    R.exact("thr = albedo", X.thr32 == f32(albedo))


def law_diffuse_light(R, X, emit):
    """DiffuseLight, material.rs:214-225: no scatter; emitted = emit on the front face, 0 on the back.  ray_color returns it
    (main.rs:131, 147-149): the path ends with acc = thr * emitted"""
    R.exact("status ENDED", X.status == ENDED)
    R.exact("lobe", X.lobe == ffi.VK_MAT_DIFFUSE_LIGHT)
    check_ended(R, X, X.all)
    want = X.states["thr"] * f32(emit) if X.front else np.zeros((X.n, 3), f32)       # (the products are exact in f32 by choice)
    R.exact("acc = thr * emitted", X.out["state"]["acc"] == want)


def weight_identity(R, X, sel, albedo, lights, what=""):
    """main.rs:139-146 with MixturePDF::value (util.rs:172-175), CosinePDF::value (util.rs:134-142: about unit(normal), 0 for
    cos <= 0), HittablePDF over `lights` and Lambertian::scattering_pdf (material.rs:100-108; Isotropic's is the same, :456-464: the
    normal AS GIVEN against the unit direction, 0 for cos < 0):  thr = albedo * spdf(d) / pdf(d), from the returned f32 direction in
    f64.  spdf = 0 over a positive pdf is exactly 0; 0 over 0 is NaN (kept: main.rs:192-196 filters it per sample)."""
    d = X.d[sel]
    dh, nh = unit(d), unit(X.normal)
    cos_given, cos_unit = dot(X.normal, dh), dot(nh, dh)
    spdf = np.where(cos_given < 0.0, 0.0, cos_given / math.pi)
    light, unstable = lights_pdf(lights, X.p, d)
    pdf = 0.5 * light + 0.5 * np.where(cos_unit <= 0.0, 0.0, cos_unit / math.pi)
    unstable = unstable | ((np.abs(cos_unit) < COS_MIN) & (cos_unit != 0.0))
    R.exclude(unstable)
    ok = ~unstable
    thr = X.thr[sel]
    nan = ok & (pdf == 0.0) & (spdf == 0.0)
    zero = ok & (pdf > 0.0) & (spdf == 0.0)
    pos = ok & (pdf > 0.0) & (spdf > 0.0)
    R.exact(f"{what}every stable sample is NaN, 0 or positive", (nan | zero | pos)[ok])
    R.exact(f"{what}thr is NaN for exactly the 0 / 0 items", np.isnan(thr).all(1)[ok] == nan[ok])
    R.exact(f"{what}thr = 0 where spdf = 0 < pdf", thr[zero] == 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.asarray(albedo, f64)[None, :] * (spdf / pdf)[:, None]
        R.ident(f"{what}thr = albedo spdf / pdf (relative)", (thr[pos] / want[pos] - 1.0), TOL_WEIGHT)
    return dict(light=light, pdf=pdf, spdf=spdf, ok=ok, pos=pos, nan=nan, zero=zero, want=want)


def cosine_branch(R, d, nh, what=""):
    """CosinePDF::generate, util.rs:52-63, 144-146 about ONB::new_from_w(normal) (util.rs:95-110): z = sqrt(1 - r2), the disc radius
    sqrt(r2): unit length, density cos / pi.  E[cos] = 2/3, E[cos^2] = 1/2, nothing across the axis.  Control: the uniform hemisphere
    (1/2 and 1/3)."""
    t1, t2 = tangents(nh)
    c = dot(d, nh)
    R.ident(f"{what}|d| = 1", np.sqrt(dot(d, d)) - 1.0, TOL_UNIT)
    R.mean(f"{what}cosine branch: E[d . n]", c, 2.0 / 3.0, 1.0 / 2.0)
    R.mean(f"{what}cosine branch: E[d . t1]", dot(d, t1), 0.0)
    R.mean(f"{what}cosine branch: E[d . t2]", dot(d, t2), 0.0)
    R.mean(f"{what}cosine branch: E[cos^2]", c * c, 1.0 / 2.0, 1.0 / 3.0)
    R.exact(f"{what}cosine branch: d . n > 0", c > 0.0)


def rect_branch(R, q, rect, what=""):
    """Rect::random, hittable.rs:284-292: the point q = d + origin is uniform on the rect: in its plane, inside its extents, mean the
    centre, variance side^2 / 12 per axis.  Control: the two sampled axes exchanged (the other side's variance)."""
    a0, a1, a2 = rect.axes
    R.ident(f"{what}light point in its rect's plane", q[:, a2] - rect.k, TOL_UNIT)
    R.exact(f"{what}light point inside the extents", rect.inside(q, TOL_UNIT))
    s0, s1 = rect.c1 - rect.c0, rect.d1 - rect.d0
    m0, m1 = (rect.c0 + rect.c1) / 2.0, (rect.d0 + rect.d1) / 2.0
    differ = abs(s0 - s1) > 0.2 * max(s0, s1)
    R.mean(f"{what}light point: mean axis0", q[:, a0], m0)
    R.mean(f"{what}light point: mean axis1", q[:, a1], m1)
    R.mean(f"{what}light point: variance axis0", (q[:, a0] - m0) ** 2, s0 * s0 / 12.0, s1 * s1 / 12.0 if differ else None)
    R.mean(f"{what}light point: variance axis1", (q[:, a1] - m1) ** 2, s1 * s1 / 12.0, s0 * s0 / 12.0 if differ else None)


def law_diffuse_pdf(R, X, sel, albedo, lobe, scene, branch, what=""):
    """Lambertian (material.rs:92-108) or Isotropic (:448-464) under the PDF integrator, main.rs:139-146: the direction comes from
    MixturePDF(lights 0.5, cosine 0.5).generate (util.rs:177-185), the light half from Vec::random over `lights` (hittable.rs:429-433),
    the weight is attenuation * scattering_pdf / pdf, r.time is kept.  Control: the mixture at 0.25 / 0.75 — in value AND generate an
    unbiased estimator that no expectation can tell from the reference's.
    branch(R, X, sel, w) -> the light-branch mask (over all items), or None where the case cannot tell the branches apart."""
    check_scattered(R, X, sel, lobe, X.time_in, what)
    w = weight_identity(R, X, sel, albedo, scene.lights, what)
    mask = branch(R, X, sel, w)
    if mask is None:
        return
    count = int(sel.sum())
    R.share(f"{what}light branch share", sel & mask, count, 0.5, 0.25)
    cosine_branch(R, X.d[sel & ~mask], unit(X.normal), what)


# ---- how a case tells the mixture's branches apart
def branch_by_length(scene):
    """every point of every light is farther than 1.5 from p: a light-branch direction (point - origin, not normalised) is longer than
    1.5 or the default draw (1, 0, 0) exactly; a cosine-branch direction has unit length"""
    def branch(R, X, sel, w):
        length = np.sqrt(dot(X.d, X.d))
        default = (X.out["next"]["direction"] == f32([1.0, 0.0, 0.0])).all(1)
        far = length > 1.5
        R.exact("a direction is a unit vector or longer than 1.5", (far | (np.abs(length - 1.0) < TOL_UNIT))[sel])
        light = sel & (far | default)
        scene.light_branch(R, X, sel, light, default, w)
        return light
    return branch


def _rect_scene_branch(scene):
    def light_branch(R, X, sel, light, default, w):
        R.exact("no default draw", ~default[sel])
        rect_branch(R, X.d[light] + X.p, scene.lights[0])
    return light_branch


# ================================================================ scenes
ALB_LAM, ALB_MET, ALB_MIRROR, ALB_MIRROR_B, ALB_ISO = (0.25, 0.5, 0.75), (0.875, 0.75, 0.5), (0.5, 0.625, 0.375), (0.125, 0.25, 0.0625), \
    (0.75, 0.375, 0.5)
EMIT, THR_LIGHT = (4.0, 2.0, 1.0), (0.5, 0.25, 2.0)
FUZZ, REF_IDX = 0.5, 1.5
M_LAM, M_MET, M_MIRROR, M_GLASS, M_ISO, M_LIGHT, M_MIRROR_B, M_SPEC_IN, M_SPEC, M_NEST = range(10)
PCT, PCT_IN = 0.3, 0.5


class Scene:
    """a description, its `lights` as plain numbers and how a light-branch sample of it is checked"""

    def __init__(self, name, lights, light_branch, with_spec):
        self.name, self.lights, self.with_spec = name, lights, with_spec
        self.light_branch = light_branch(self)
        self._built = None

    def desc(self):
        """(owner, desc), built once per process"""
        if self._built is None:
            d = Desc()
            ids = [d.lambertian(*ALB_LAM), d.mat(ffi.VK_MAT_METAL, d.solid(*ALB_MET), FUZZ), d.mat(ffi.VK_MAT_METAL, d.solid(*ALB_MIRROR), 0.0),
                   d.mat(ffi.VK_MAT_DIELECTRIC, d.solid(1, 1, 1), REF_IDX), d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(*ALB_ISO)), d.light(*EMIT)]
            if self.with_spec:            # (the scatter integrator refuses a description that holds a SpecDiffuse)
                ids.append(d.mat(ffi.VK_MAT_METAL, d.solid(*ALB_MIRROR_B), 0.0))
                ids.append(d.mat(ffi.VK_MAT_SPEC_DIFFUSE, 0, PCT_IN, M_MIRROR_B, M_LAM))
                ids.append(d.mat(ffi.VK_MAT_SPEC_DIFFUSE, 0, PCT, M_MIRROR, M_LAM))
                ids.append(d.mat(ffi.VK_MAT_SPEC_DIFFUSE, 0, PCT, M_MIRROR, M_SPEC_IN))
            assert ids == list(range(len(ids)))
            refs = [l.add(d) for l in self.lights]
            # a real world for the traced pair: a Lambertian floor under the lights and a Metal one far to the side
            world = [d.xz_rect(-50, 50, -50, 50, 0.0, M_LAM), d.xz_rect(100, 120, -10, 10, -5.0, M_MET)]
            world = d.list_(world + [r for l, r in zip(self.lights, refs) if not isinstance(l, BoxL)])
            for l, r in zip(self.lights, refs):
                if isinstance(l, BoxL):                   # (a list may not hold a list)
                    world = d.big_box(world, r)
            self._built = (d, d.finish(world, refs))
        return self._built


RECT = RectL(-0.5, 0.5, -0.75, 0.75, 2.0, (0, 2, 1))              # an xz rect, sides 1 and 1.5, at height 2
P_RECT = (-1.25, 0.0, 0.25)                                       # the nearest point of RECT is sqrt(0.75^2 + 2^2) = 2.14 away

# six entries; every plane has a coordinate of its own (x: -5, 2.5, 1.5; y: 3, 2.5, 2, 3.5; z: 4, -6, -7) and no rect is square or
# centred on an axis, so that two exchanged axes leave the extents
ZOO_RECTS = [RectL(-1.0, 0.5, 0.25, 1.0, 3.0, (0, 2, 1)), RectL(0.5, 2.0, 1.0, 1.5, 4.0, (0, 1, 2)), RectL(0.5, 1.0, -2.0, -0.5, -5.0, (1, 2, 0))]
ZOO_BOX = BoxL((1.5, 2.0, -7.0), (2.5, 2.5, -6.0))
ZOO = ZOO_RECTS + [ZOO_BOX,
                   DefaultL(lambda d: Desc.flip(d.rect(-3.0, -2.0, 1.0, 2.0, 3.5, (0, 2, 1), d.light(0, 0, 0)))),
                   DefaultL(lambda d: d.moving_sphere((0.0, 6.0, 0.0), (0.5, 6.0, 0.0), 0.0, 1.0, 1.0, d.light(0, 0, 0)))]
P_ZOO = (0.0, 0.0, 0.0)


def _zoo_branch(scene):
    """Vec::random, hittable.rs:429-433: an entry chosen evenly, 1 / (2 k) of all samples each; a Boxy spends its share evenly on its
    six sides (:375-377), three of which, with the FlipFace'd entry and the MovingSphere, answer (1, 0, 0).  Control: entry 0 always."""
    def light_branch(R, X, sel, light, default, w):
        k, count = len(scene.lights), int(sel.sum())
        q = X.d + X.p
        planes = [(f"rect {i}", r, 1.0 / (2 * k)) for i, r in enumerate(ZOO_RECTS)] + \
                 [(f"box side {i}", r, 1.0 / (12 * k)) for i, r in enumerate(ZOO_BOX.plain)]
        # a point within the tolerance of a Boxy's edge is inside two of its sides: it belongs to the plane it is nearest to
        gap = np.stack([np.where(r.inside(q, TOL_UNIT), np.abs(q[:, r.axes[2]] - r.k), np.inf) for _, r, _ in planes])
        nearest, hits = gap.argmin(0), np.isfinite(gap).any(0).astype(int)
        for i, (name, rect, share) in enumerate(planes):
            on = light & ~default & (hits == 1) & (nearest == i)
            R.share(f"share of {name}", on, count, share, 0.5 if i == 0 else None)
            a0, a1, _ = rect.axes
            R.mean(f"{name}: mean axis0", q[on][:, a0], (rect.c0 + rect.c1) / 2.0)
            R.mean(f"{name}: mean axis1", q[on][:, a1], (rect.d0 + rect.d1) / 2.0)
        R.exact("a light-branch point lies on a plane of `lights`", hits[light & ~default] == 1)
        R.share("share of the default draw (1, 0, 0)", light & default, count, (2.0 + 3.0 / 6.0) / (2 * k))
        R.exact("the default draw has light pdf 0", w["light"][(light & default)[sel]] == 0.0)
    return light_branch


SPHERE_AWAY = SphereL((0.5, -3.0, 0.25), 1.0)                     # below the horizon of the normal +y at the origin
SPHERE_OVER = SphereL((0.5, 3.0, 0.25), 1.0)
P_SPHERE = (0.0, 0.0, 0.0)


def _no_branch(scene):
    return lambda *a: None


SCENES = {
    "rect": Scene("rect", [RECT], _rect_scene_branch, True),
    "rect-scatter": Scene("rect-scatter", [RECT], _rect_scene_branch, False),
    "zoo": Scene("zoo", ZOO, _zoo_branch, True),
    "sphere-away": Scene("sphere-away", [SPHERE_AWAY], _no_branch, True),
    "sphere-over": Scene("sphere-over", [SPHERE_OVER], _no_branch, True),
}


def branch_sphere_away(scene):
    """Sphere::random, hittable.rs:115-134, in the frame of w = unit(centre - p): z = d . w uniform on [cos_max, 1], the part across w of
    length 1 - z^2 (NOT its root: the reference's own, kept), azimuth uniform.  |d|^2 = z^2 + (1 - z^2)^2 approaches 1, so the length
    does not separate the branches; here the hemisphere is turned away from the cone: every light-branch sample has weight exactly 0
    and every cosine-branch direction has z < cos_max.  Control: the textbook cone, sqrt(1 - z^2)."""
    sph = scene.lights[0]

    def branch(R, X, sel, w):
        light = np.zeros(X.n, bool)
        light[sel] = (X.thr[sel] == 0.0).all(1)
        wv = unit(sph.center - X.p)
        cm = sph.cos_max(X.p)
        ez, var, e_lin, e_root = cone_moments(cm)
        z = dot(X.d, wv)
        R.exact("a cosine-branch direction misses the cone", z[sel & ~light] < cm)
        R.exact("a cosine-branch weight is 2 albedo", np.abs(X.thr[sel & ~light] / (2.0 * np.asarray(ALB_LAM)) - 1.0) <= ULP4)
        zl, dl = z[light], X.d[light]
        across = dl - zl[:, None] * wv
        length = np.sqrt(dot(across, across))
        R.exact("z within [cos_max, 1]", (zl >= cm - TOL_UNIT) & (zl <= 1.0 + TOL_UNIT))
        R.ident("|d - z w| = 1 - z^2", length - (1.0 - zl * zl), TOL_UNIT)
        R.mean("cone: E[z]", zl, ez)
        R.mean("cone: Var[z]", (zl - ez) ** 2, var)
        R.mean("cone: E|d - z w|", length, e_lin, e_root)
        t1, t2 = tangents(wv)
        R.mean("cone: E[d . t1]", dot(dl, t1), 0.0)
        R.mean("cone: E[d . t2]", dot(dl, t2), 0.0)
        return light
    return branch


# ================================================================ cases
class Case:
    def __init__(self, name, scene, integrator, seed, p, normal, front, material, d_in, law, thr=(1.0, 1.0, 1.0), medium=0):
        self.name, self.scene, self.integrator, self.seed, self.law = name, SCENES[scene], integrator, seed, law
        self.p, self.normal, self.front, self.material, self.d_in, self.thr, self.medium = p, normal, front, material, d_in, thr, medium
        length = math.sqrt(sum(x * x for x in d_in))
        assert 0.7 <= length <= 3.0 and abs(length - 1.0) > 0.05, "the incoming direction is not unit length"

    def items(self, n=N, seed=None):
        """(rays, hits, states): n items that differ in their stream alone"""
        p, d_in = np.asarray(self.p, f32), np.asarray(self.d_in, f32)
        rays = make_rays(np.tile(p - d_in, (n, 1)), np.tile(d_in, (n, 1)), TIME)
        hits = np.zeros(n, HIT_DTYPE)
        hits["p"], hits["t"], hits["normal"], hits["u"], hits["v"] = p, 1.0, np.asarray(self.normal, f32), 0.5, 0.25
        hits["hit"], hits["front"], hits["material"], hits["medium"] = 1, int(self.front), self.material, self.medium
        hits["object"] = ffi.make_ref(ffi.VK_KIND_RECT, 0)          # (the floor; a bounce does not read it)
        states = make_path_states(n, self.seed if seed is None else seed)
        states["thr"] = np.asarray(self.thr, f32)
        return rays, hits, states

    def kwargs(self):
        return dict(max_depth=50, integrator=self.integrator, background=ffi.VK_BACKGROUND_SOLID, background_color=BACKGROUND)

    def check(self, out, rays, hits, states, has_lobe=True):
        """the whole rule on one bounce's results: a Report, finished by the caller"""
        R, X = Report(self.name), Out(out, rays, hits, states, has_lobe)
        check_copied(R, X)
        self.law(R, X, self)
        return R


def _u(v):
    return tuple(float(x) for x in unit(v))


def _incoming(cos, length, normal=(0.0, 1.0, 0.0)):
    """a direction of that length whose unit vector has the cosine -cos against the unit normal"""
    nh = unit(normal)
    t1, _ = tangents(nh)
    return tuple(float(x) for x in length * (math.sqrt(1.0 - cos * cos) * t1 - cos * nh))


D_IN = (0.5, -1.5, 0.25)           # length 1.6
UP = (0.0, 1.0, 0.0)
ONB_NORMALS = [(1.0, 0.0, 0.0), _u((0.95, 0.2, 0.1)), _u((0.85, 0.4, 0.2)), _u((-0.99, 0.05, 0.0))]      # both sides of |w.x| > 0.9


def _diffuse(albedo, lobe, branch):
    return lambda R, X, c: law_diffuse_pdf(R, X, X.all, albedo, lobe, c.scene, branch(c.scene))


def law_twice_the_normal(R, X, c):
    """a normal of length 2 under the PDF integrator: CosinePDF normalises it (util.rs:100), scattering_pdf does not (material.rs:101):
    the weight doubles, and a cosine-branch direction that misses the light carries (2 cos / pi) / (cos / 2 pi) = 4 albedo"""
    law_diffuse_pdf(R, X, X.all, ALB_LAM, ffi.VK_MAT_LAMBERTIAN, c.scene, branch_by_length(c.scene))
    light, _ = lights_pdf(c.scene.lights, X.p, X.d)
    missed = (np.abs(np.sqrt(dot(X.d, X.d)) - 1.0) < TOL_UNIT) & (light == 0.0) & (dot(unit(X.d), unit(X.normal)) >= COS_MIN)
    R.exact("some cosine-branch directions miss the light", missed.sum() > X.n // 8)
    R.exact("such a direction carries 4 albedo", np.abs(X.thr[missed] / (4.0 * np.asarray(ALB_LAM)) - 1.0) <= ULP4)


def law_zoo_tilted(R, X, c):
    """the normal tilted towards +x: the default draw (1, 0, 0) meets nothing in `lights`, its light pdf is 0 and its cosine positive:
    (cos / pi) / (cos / 2 pi) = 2 albedo"""
    law_diffuse_pdf(R, X, X.all, ALB_LAM, ffi.VK_MAT_LAMBERTIAN, c.scene, branch_by_length(c.scene))
    default = (X.out["next"]["direction"] == f32([1.0, 0.0, 0.0])).all(1)
    R.exact("a default draw carries 2 albedo", np.abs(X.thr[default] / (2.0 * np.asarray(ALB_LAM)) - 1.0) <= ULP4)


def law_zoo_level(R, X, c):
    """the normal +y: n . (1, 0, 0) = 0 and the light pdf is 0: 0 / 0, NaN for exactly the default draws"""
    law_diffuse_pdf(R, X, X.all, ALB_LAM, ffi.VK_MAT_LAMBERTIAN, c.scene, branch_by_length(c.scene))
    default = (X.out["next"]["direction"] == f32([1.0, 0.0, 0.0])).all(1)
    R.exact("thr is NaN for exactly the default draws", np.isnan(X.thr).all(1) == default)
    R.exact("no channel of another item is NaN", ~np.isnan(X.thr[~default]).any())


def law_spec_diffuse(R, X, c):
    """SpecDiffuse, material.rs:474-487: rng < pct takes the specular child's scatter_with_pdf, else the diffuse child's; scattering_pdf
    is the diffuse child's.  Metal fuzz 0 over Lambertian, pct 0.3: shares 0.3 / 0.7, each lobe under its own law (Metal's specular ray
    has time 0, Lambertian's keeps r.time).  Control: the children exchanged (0.7)."""
    metal = X.lobe == ffi.VK_MAT_METAL
    R.share("share of the specular child", metal, X.n, PCT, 1.0 - PCT)
    law_metal(R, X, metal, ALB_MIRROR, 0.0, PDF, "specular: ")
    law_diffuse_pdf(R, X, ~metal, ALB_LAM, ffi.VK_MAT_LAMBERTIAN, c.scene, branch_by_length(c.scene), "diffuse: ")


def law_spec_nested(R, X, c):
    """pct 0.3 over pct 0.5: the outer mirror 0.3, the inner mirror and the Lambertian 0.35 each; the mirrors differ in their albedo"""
    metal = X.lobe == ffi.VK_MAT_METAL
    outer = metal & (X.thr32 == f32(ALB_MIRROR)).all(1)
    inner = metal & (X.thr32 == f32(ALB_MIRROR_B)).all(1)
    R.exact("a specular sample carries one of the two mirrors' albedos", (outer | inner)[metal])
    R.share("share of the outer mirror", outer, X.n, PCT, 1.0 - PCT)
    R.share("share of the inner mirror", inner, X.n, (1.0 - PCT) * PCT_IN, PCT_IN)
    law_metal(R, X, outer, ALB_MIRROR, 0.0, PDF, "outer: ")
    law_metal(R, X, inner, ALB_MIRROR_B, 0.0, PDF, "inner: ")
    law_diffuse_pdf(R, X, ~metal, ALB_LAM, ffi.VK_MAT_LAMBERTIAN, c.scene, branch_by_length(c.scene), "diffuse: ")


def _cases():
    seed = iter(range(101, 1000))
    lam_pdf = _diffuse(ALB_LAM, ffi.VK_MAT_LAMBERTIAN, branch_by_length)
    metal = lambda fuzz, integ, alb: (lambda R, X, c: law_metal(R, X, X.all, alb, fuzz, integ))
    graze = _incoming(0.2, 1.7)
    glass = [("front-cos0.9", True, 0.9, None), ("front-cos0.5", True, 0.5, "r0"), ("front-cos0.2", True, 0.2, "r0"),
             ("back-cos0.8", False, 0.8, "transmitted"), ("back-total", False, 0.5, None)]
    out = []
    for integ, scene in ((SCATTER, "rect-scatter"), (PDF, "rect")):
        tag = INTEG_NAME[integ]
        if integ == SCATTER:
            lam = lambda R, X, c: law_lambertian_scatter(R, X, ALB_LAM)
            out.append(Case("lambertian-scatter", scene, integ, next(seed), P_RECT, UP, True, M_LAM, D_IN, lam))
            out.append(Case("lambertian-scatter-normal2", scene, integ, next(seed), P_RECT, (0.0, 2.0, 0.0), True, M_LAM, D_IN, lam))
            out.append(Case("isotropic-scatter", scene, integ, next(seed), P_RECT, (1.0, 0.0, 0.0), True, M_ISO, D_IN,
                            lambda R, X, c: law_isotropic_scatter(R, X, ALB_ISO), medium=1))
        else:
            out.append(Case("lambertian-pdf-rect", scene, integ, next(seed), P_RECT, UP, True, M_LAM, D_IN, lam_pdf))
            out.append(Case("lambertian-pdf-rect-normal2", scene, integ, next(seed), P_RECT, (0.0, 2.0, 0.0), True, M_LAM, D_IN,
                            law_twice_the_normal))
            for i, n in enumerate(ONB_NORMALS):
                out.append(Case(f"lambertian-pdf-rect-onb{i}", scene, integ, next(seed), P_RECT, n, True, M_LAM, D_IN, lam_pdf))
            out.append(Case("isotropic-pdf", scene, integ, next(seed), P_RECT, (1.0, 0.0, 0.0), True, M_ISO, D_IN,
                            _diffuse(ALB_ISO, ffi.VK_MAT_ISOTROPIC, branch_by_length), medium=1))
            out.append(Case("spec-diffuse", scene, integ, next(seed), P_RECT, UP, True, M_SPEC, D_IN, law_spec_diffuse))
            out.append(Case("spec-diffuse-nested", scene, integ, next(seed), P_RECT, UP, True, M_NEST, D_IN, law_spec_nested))
        out.append(Case(f"metal-fuzz-{tag}", scene, integ, next(seed), P_RECT, UP, True, M_MET, graze, metal(FUZZ, integ, ALB_MET)))
        out.append(Case(f"metal-mirror-{tag}", scene, integ, next(seed), P_RECT, UP, True, M_MIRROR, graze, metal(0.0, integ, ALB_MIRROR)))
        for name, front, cos, control in glass:
            out.append(Case(f"dielectric-{name}-{tag}", scene, integ, next(seed), P_RECT, UP, front, M_GLASS, _incoming(cos, 1.3),
                            lambda R, X, c, control=control: law_dielectric(R, X, REF_IDX, control)))
        for front in (True, False):
            out.append(Case(f"light-{'front' if front else 'back'}-{tag}", scene, integ, next(seed), P_RECT, UP, front, M_LIGHT, D_IN,
                            lambda R, X, c: law_diffuse_light(R, X, EMIT), thr=THR_LIGHT))
    out.append(Case("zoo-level", "zoo", PDF, next(seed), P_ZOO, UP, True, M_LAM, D_IN, law_zoo_level))
    out.append(Case("zoo-tilted", "zoo", PDF, next(seed), P_ZOO, _u((0.5, 1.0, 0.1)), True, M_LAM, D_IN, law_zoo_tilted))
    out.append(Case("sphere-light-away", "sphere-away", PDF, next(seed), P_SPHERE, UP, True, M_LAM, D_IN,
                    _diffuse(ALB_LAM, ffi.VK_MAT_LAMBERTIAN, branch_sphere_away)))
    out.append(Case("sphere-light-overhead", "sphere-over", PDF, next(seed), P_SPHERE, UP, True, M_LAM, D_IN,
                    _diffuse(ALB_LAM, ffi.VK_MAT_LAMBERTIAN, lambda scene: (lambda *a: None))))
    return out


CASES = {c.name: c for c in _cases()}
SEEDS = {c.name: c.seed for c in CASES.values()}
SECOND_SEED = 7001                 # of the one repeat at 4 N that a failing statistic gets


def batches():
    """(scene name, integrator) -> the cases that one interleaved vk_shade_hits call can hold"""
    out = {}
    for c in CASES.values():
        out.setdefault((c.scene.name, c.integrator), []).append(c.name)
    return out


N_EXTRA = 77                       # misses appended to an interleaved batch: its length is no multiple of 256
BACKGROUND = (0.25, 0.5, 0.125)


def _rows(a):
    """a record array as rows of 32-bit words (numpy moves those far faster than records)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


def interleaved(names, n=N, parts=None):
    """the items of the named cases (parts: their items() where the caller has them) and N_EXTRA misses, interleaved by a fixed
    permutation: (rays, hits, states, perm, slices); unpermute(result, perm)[slices[name]] are that case's results in its own order,
    slices[None] the misses'"""
    parts = [CASES[name].items(n) for name in names] if parts is None else [p[:3] for p in parts]
    extra = CASES[names[0]].items(N_EXTRA, seed=9)
    extra[1]["hit"] = 0
    total = len(names) * n + N_EXTRA
    perm = np.random.default_rng(20240).permutation(total)
    out = []
    for i, dtype in enumerate((RAY_DTYPE, HIT_DTYPE, PATH_STATE_DTYPE)):
        whole = np.concatenate([_rows(p[i]) for p in parts] + [_rows(extra[i])])
        out.append(whole[perm].view(dtype).reshape(total))
    slices = {name: slice(i * n, (i + 1) * n) for i, name in enumerate(names)}
    slices[None] = slice(len(names) * n, total)
    return out[0], out[1], out[2], perm, slices


def unpermute(a, perm):
    """the inverse of interleaved()'s order: out[perm[i]] = a[i]"""
    rows = _rows(a)
    out = np.empty_like(rows)
    out[perm] = rows
    return out.view(a.dtype).reshape(len(a))


def check_misses(out, states):
    """main.rs:150-152 with the solid background: acc += thr * background, nothing drawn"""
    assert (out["status"] == MISS).all() and (out["lobe"] == 0xFFFFFFFF).all() and not np.ascontiguousarray(out["next"]).view(np.uint32).any()
    assert (out["state"]["acc"] == states["thr"] * f32(BACKGROUND)).all() and (out["state"]["counter"] == states["counter"]).all()


# ================================================================ the traced pair
def traced_rays(which, n=N):
    """n copies of one ray aimed at a real floor of the `rect` scenes' world — the Lambertian floor at P_RECT under the light, the Metal
    floor at an incidence cosine of 0.2 — so that the library's own walk writes the records (oriented normal, front, material)"""
    if which == "lambertian":
        d_in, p = np.asarray(D_IN, f64), np.asarray(P_RECT, f64)
    else:
        d_in, p = np.asarray(_incoming(0.2, 1.7), f64), np.array([110.0, -5.0, 0.5])
    return make_rays(np.tile(p - d_in, (n, 1)), np.tile(d_in, (n, 1)), TIME)


TRACED = {"lambertian": ("rect", PDF, 801, "lambertian-pdf-rect"), "metal": ("rect-scatter", SCATTER, 802, "metal-fuzz-scatter")}
