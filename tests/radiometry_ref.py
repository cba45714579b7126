"""Closed-form radiometry for the integrators.  TESTS ONLY; shared by tests/test_radiometry.py (oracle, emulator) and
tests/test_gpu_radiometry.py (the public ABI on the device).

Everything here is plain f64 numpy and shares nothing with the library's restatement of the reference: no import of the oracle or an
emulator, no formula taken from vk_trace.h.  From vecchio_amd only the ffi constants and record types that tests/descs.py needs to
write a scene down.  Every expected value cites the reference's own lines (main.rs, material.rs, hittable.rs, util.rs).

The statistical rule (the same for every case and route):
  * a per-sample route (oracle, emulator, the debug hooks) gives samples x_1..x_n: mean, SE = s / sqrt(n).  A non-finite sample counts
    as 0 and stays in n (main.rs:192-196 drops it from the sum, not from the divisor);
  * a public call gives one mean per submitted copy of the same ray or point (first_index gives each copy its own stream): the mean of
    the R >= 256 replica means, SE = their spread / sqrt(R);
  * |mean - want| <= 4 SE + ROUND * |want| per channel, and SE <= SE_CAP * |want| so that no pass comes from a vacuous SE;
  * every family has a power control: a plausible wrong value that the same data must reject by |z| > 4.
ROUND is not statistical: a case whose samples are all equal (the blue channel behind the glass ball, the mirror) has SE = 0, and what
is left is f32 rounding of the sky's lerp and of the mean (a few ulp, 6e-8 each)."""
import math

import numpy as np

from descs import Desc, camera, params  # noqa: F401  (camera, params: re-exported for the tests)
from vecchio_amd import ffi

f64 = np.float64
Z_MAX = 4.0
SE_CAP = 0.005            # a condition, not a measurement
SE_AIM = 0.0045           # a count whose measured SE lands above this is raised
ROUND = 1e-6              # f32 rounding of a mean of equal samples: ~16 ulp of 2^-24


# ================================================================ closed forms
def _corner(a, b, h):
    """form factor of an a x b rectangle at height h over an element below one of its corners (odd in a and in b)"""
    A, B = a / h, b / h
    sa, sb = math.sqrt(1.0 + A * A), math.sqrt(1.0 + B * B)
    return (A / sa * math.atan(B / sa) + B / sb * math.atan(A / sb)) / (2.0 * math.pi)


def rect_form_factor_parallel(x0, z0, rect, h):
    """cosine-weighted form factor  int cos cos' / (pi r^2) dA = int h^2 / (pi r^4) dA  of the horizontal rectangle
    rect = (xa, xb, za, zb) at height h above a horizontal element at (x0, z0): four corner terms superposed"""
    xa, xb, za, zb = (float(v) for v in rect)
    return (_corner(xb - x0, zb - z0, h) - _corner(xa - x0, zb - z0, h) - _corner(xb - x0, za - z0, h) + _corner(xa - x0, za - z0, h))


def polygon_form_factor(p, n, verts):
    """Lambert's edge formula |sum_i gamma_i (Gamma_i . n)| / (2 pi) for a polygon seen from the element at p with normal n: gamma_i the
    angle the i-th edge subtends at p, Gamma_i the unit normal of the plane through p and that edge.  Valid while the whole polygon is
    above the element's horizon."""
    p, n = np.asarray(p, f64), np.asarray(n, f64)
    n = n / np.linalg.norm(n)
    r = np.asarray(verts, f64) - p
    assert (r @ n > 0).all(), "polygon_form_factor: the polygon crosses the element's horizon"
    r = r / np.linalg.norm(r, axis=1, keepdims=True)
    total = 0.0
    for i in range(len(r)):
        a, b = r[i], r[(i + 1) % len(r)]
        c = np.cross(a, b)
        total += math.atan2(np.linalg.norm(c), float(a @ b)) * float(c @ n) / np.linalg.norm(c)
    return abs(total) / (2.0 * math.pi)


def quadrature_parallel(x0, z0, rect, h, m=4000, power=4):
    """midpoint rule on an m x m grid of  h^(power-2) / (pi r^power)  over the rectangle: power 4 is the form factor, power 3 the same
    integral WITHOUT the receiver's cosine (the power control of the rect family)"""
    xa, xb, za, zb = rect
    x = xa + (np.arange(m) + 0.5) * ((xb - xa) / m) - x0
    z = za + (np.arange(m) + 0.5) * ((zb - za) / m) - z0
    r2 = x[:, None] ** 2 + z[None, :] ** 2 + h * h
    return float((h ** (power - 2) / (math.pi * r2 ** (power / 2))).sum() * ((xb - xa) / m) * ((zb - za) / m))


def integrating_sphere(a, f, Le, D):
    """radiance arriving, cosine-weighted, at the wall of a Lambertian sphere of albedo a around a lamp of radiance Le that fills the
    share f of every wall point's cosine-weighted directions, within D path segments:  Le f (1 - q^D) / (1 - q), q = a (1 - f).
    Segment 1 meets the lamp with probability f (DiffuseLight::emitted, material.rs:218-225; it does not scatter, :215-217); otherwise it
    meets the wall, which reflects a of what ITS hemisphere receives within D - 1 segments (Lambertian, material.rs:85-108: cosine
    sampling with scattering_pdf cos / pi cancels to the albedo).  ray_color(depth) returns 0 once depth > MAX_DEPTH, main.rs:126-128, and
    the first call has depth 1 (main.rs:190): D segments."""
    a, Le = np.asarray(a, f64), np.asarray(Le, f64)
    q = a * (1.0 - f)
    return Le * f * (1.0 - q ** D) / (1.0 - q)


def glass_diameter_chain(R0, D):
    """(P_back, P_fwd) of a ray along a glass ball's diameter within D segments.  At normal incidence schlick() is r0 whatever the side
    (util.rs:25-29 at cosine 1; r0 is the same for n and 1 / n), refract() keeps the direction (util.rs:18-23) and reflect() reverses it
    (util.rs:14-16): three states (outside going back, inside going up, inside going down).  Segment 1 ends on the ball; reflected
    there (R0) the path leaves backwards with segment 2; transmitted (1 - R0) it crosses the ball, segment 2, and at each further
    interface leaves (1 - R0) with one more segment or turns round (R0): after k inner reflections it leaves with segment 3 + k, forwards
    for even k, backwards for odd k.  A path that has not left within D segments returns 0 (main.rs:126-128)."""
    back = R0 if D >= 2 else 0.0
    fwd = 0.0
    for k in range(0, max(0, D - 2)):            # 3 + k <= D
        p = (1.0 - R0) * R0 ** k * (1.0 - R0)
        if k % 2 == 0:
            fwd += p
        else:
            back += p
    return back, fwd


def sky(direction):
    """main.rs's In-One-Weekend background: lerp of white and (0.5, 0.7, 1) by t = (unit(d).y + 1) / 2 (VK_BACKGROUND_SKY)"""
    d = np.asarray(direction, f64)
    t = 0.5 * (d[1] / np.linalg.norm(d) + 1.0)
    return (1.0 - t) * np.ones(3) + t * np.array([0.5, 0.7, 1.0])


def clean(samples):
    """(n, 3) f64 with every non-finite SAMPLE (any channel) set to 0 and kept in n, as main.rs:192-196 and the library do"""
    x = np.asarray(samples, f64).reshape(-1, 3)
    bad = ~np.isfinite(x).all(1)
    x = x.copy()
    x[bad] = 0.0
    return x, int(bad.sum())


def z_scores(x, want):
    """(mean, se, z) per channel of samples — or replica means — x (n, 3) against want: se = s / sqrt(n), z = (mean - want) / se (0
    where both the difference and se are 0, inf where only se is)"""
    x, _ = clean(x)
    want = np.broadcast_to(np.asarray(want, f64), (3,))
    mean = x.mean(0)
    se = x.std(0, ddof=1) / math.sqrt(len(x))
    diff = mean - want
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(np.abs(diff) <= ROUND * np.abs(want), 0.0, diff / se)
    return mean, se, z


def check(x, want, what, control=None):
    """the rule of this module's docstring for samples or replica means x (n, 3); returns (mean, se, z) for the caller to print"""
    want = np.broadcast_to(np.asarray(want, f64), (3,))
    mean, se, z = z_scores(x, want)
    assert (se <= SE_CAP * np.abs(want)).all(), f"{what}: SE {se} above {SE_CAP} of {want}: the comparison would be vacuous"
    assert (np.abs(mean - want) <= Z_MAX * se + ROUND * np.abs(want)).all(), f"{what}: mean {mean} want {want} se {se} z {z}"
    if control is not None:
        control = np.broadcast_to(np.asarray(control, f64), (3,))
        differs = np.abs(control - want) > 1e-3 * np.abs(want)        # (a channel the control leaves alone cannot reject it)
        _, _, zc = z_scores(x, control)
        assert differs.any() and (np.abs(zc[differs]) > Z_MAX).all(), f"{what}: the power control {control} is not rejected, z {zc}"
    return mean, se, z


# ================================================================ cases
class Case:
    """One closed-form comparison.  route: 'rays' (radiance along rays), 'points' (irradiance at points) or 'frame' (vk_render).
    items: the submitted vk_ray records ('rays' / 'points'), group[i] the index into want / control of items[i]; 'frame': cam, w, h and
    want (h, w, 3), each pixel normalised by its own value so that every pixel is a replica of expectation (1, 1, 1).
    spp: samples per submitted record / per pixel.  kw: radiance_params()'s keywords."""

    def __init__(self, name, build, route, spp, kw, want, items=None, group=None, control=None, cam=None, size=None, flags=0):
        self.name, self.build, self.route, self.spp, self.kw = name, build, route, spp, kw
        self.want = np.asarray(want, f64)
        self.control = None if control is None else np.asarray(control, f64)
        self.items, self.group, self.cam, self.size, self.flags = items, group, cam, size, flags

    def scene(self):
        """(owner, desc): a fresh description (the owner keeps its arrays alive)"""
        owner, desc = self.build()
        desc.contents.flags = self.flags
        return owner, desc

    def render_params(self):
        w, h = self.size
        return params(w, h, self.spp, max_depth=self.kw["max_depth"], seed=self.kw["seed"], integrator=self.kw["integrator"],
                      background=self.kw["background"], bg=self.kw["background_color"])

    # ---- per-sample routes: samples (n_items, spp, >= 3) / (h * w * spp, >= 3) in render_samples' order
    def check_samples(self, samples, what=""):
        out = []
        if self.route == "frame":
            w, h = self.size
            x = np.asarray(samples, f64)[:, :3].reshape(h * w, self.spp, 3)
            return [self._check_frame(x, what)]
        x = np.asarray(samples, f64)[..., :3]
        for g in range(len(self.want)):
            out.append(self._check_group(x[self.group == g].reshape(-1, 3), g, what))
        return out

    # ---- public calls: means (n_items, 3) / an image (h, w, 3)
    def check_means(self, means, what=""):
        if self.route == "frame":
            w, h = self.size
            return [self._check_frame(np.asarray(means, f64).reshape(h * w, 1, 3), what)]
        assert np.isfinite(means).all()
        means = np.asarray(means, f64)
        out = []
        for g in range(len(self.want)):
            rep = means[self.group == g]
            assert len(rep) >= 256, f"{self.name}: {len(rep)} replicas"
            out.append(self._check_group(rep, g, what))
        return out

    def _check_group(self, x, g, what):
        what = f"{what} {self.name}[{g}]"
        want = self.want[g]
        if not want.any():                      # an exact zero (nothing can arrive within max_depth segments): every sample is 0
            assert not np.asarray(x).any(), f"{what}: expected exactly 0"
            return np.zeros(3), np.zeros(3), np.zeros(3)
        return check(x, want, what, None if self.control is None else self.control[g])

    def _check_frame(self, x, what):
        what = f"{what} {self.name}"
        want = self.want.reshape(-1, 1, 3)
        if not want.any():
            assert not np.asarray(x).any(), f"{what}: expected exactly 0"
            return np.zeros(3), np.zeros(3), np.zeros(3)
        x, _ = clean(x)
        x = x.reshape(want.shape[0], -1, 3) / want
        control = None if self.control is None else (self.control.reshape(-1, 1, 3) / want).mean((0, 1))
        return check(x.reshape(-1, 3), np.ones(3), what, control)


RAY = np.dtype(ffi.Ray)             # vk_ray: origin, tmax, direction, time


def _records(o, d):
    """vk_ray records (a ray: origin and direction; a point: position and normal) at time 0 with tmax = inf"""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    out = np.zeros(len(o), RAY)
    out["origin"], out["direction"], out["tmax"] = o, np.asarray(d, np.float32).reshape(-1, 3), np.inf
    return out


def _rays(o, d, copies):
    o, d = np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)
    return _records(np.repeat(o, copies, 0), np.repeat(d, copies, 0)), np.repeat(np.arange(len(o)), copies)


def _kw(seed, max_depth, integrator, background=ffi.VK_BACKGROUND_SOLID, bg=(0.0, 0.0, 0.0)):
    return dict(seed=seed, first_index=0, samples_per_ray=1, first_sample=0, max_depth=max_depth, integrator=integrator,
                background=background, background_color=bg)


PDF, SCATTER = ffi.VK_INTEGRATOR_PDF, ffi.VK_INTEGRATOR_SCATTER
INTEG_NAME = {PDF: "pdf", SCATTER: "scatter"}


# ---------------------------------------------------------------- the integrating sphere
SPHERE_A, SPHERE_LE, SPHERE_R, SPHERE_LAMP = (0.2, 0.5, 0.8), (1.0, 2.0, 3.0), 2.0, 1.0
# a wall point sees the lamp inside the cone sin(alpha) = r / R; the cosine-weighted share of a cone about the normal is sin^2(alpha)
SPHERE_F = (SPHERE_LAMP / SPHERE_R) ** 2
SPHERE_SEED, SPHERE_POINTS = 11, 64
SPHERE_DEPTHS = (1, 2, 3, 50)


def _bvh(d, objs):
    """a BVH over (ref, bmin, bmax) leaves: the halves of the list sorted along x, a node's box the union of its children's; a single
    object is its own leaf"""
    if len(objs) == 1:
        return objs[0]
    objs = sorted(objs, key=lambda o: o[1][0])
    left, right = _bvh(d, objs[:len(objs) // 2]), _bvh(d, objs[len(objs) // 2:])
    lo, hi = np.minimum(left[1], right[1]), np.maximum(left[2], right[2])
    return d.bvh_node(left[0], right[0], tuple(lo), tuple(hi)), lo, hi


def sphere_scene(lamp_in_lights=False, crowd=False):
    """crowd: 16 grey spheres of radius 0.3 on a ring of radius 6 OUTSIDE the wall — no path that starts inside ever meets one, every
    value stays — and the world a BVH over the 18: the lineariser keeps a tree of fewer than 16 objects as it is handed over, so only
    this world takes the rebuilt-tree routes (the default for a world of spheres, VK_SCENE_FAST_ACCEL)."""
    d = Desc()
    wall = d.sphere((0, 0, 0), SPHERE_R, d.lambertian(*SPHERE_A))
    lamp = d.sphere((0, 0, 0), SPHERE_LAMP, d.light(*SPHERE_LE))
    if not crowd:
        return d, d.finish(d.list_([wall, lamp]), [lamp] if lamp_in_lights else [])
    box = lambda c, r: (np.asarray(c, f64) - r, np.asarray(c, f64) + r)
    objs = [(wall,) + box((0, 0, 0), SPHERE_R), (lamp,) + box((0, 0, 0), SPHERE_LAMP)]
    grey = d.lambertian(0.5, 0.5, 0.5)
    for k in range(16):
        c = (6.0 * math.cos(2 * math.pi * k / 16), 0.4 * (k % 3 - 1), 6.0 * math.sin(2 * math.pi * k / 16))
        objs.append((d.sphere(c, 0.3, grey),) + box(c, 0.3))
    return d, d.finish(_bvh(d, objs)[0], [lamp] if lamp_in_lights else [])


def sphere_points(copies=4):
    """64 wall points 2u with the normal -u (u: seeded unit vectors), `copies` times each: by symmetry every one is a replica"""
    u = np.random.default_rng(SPHERE_SEED).normal(size=(SPHERE_POINTS, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u = np.tile(u, (copies, 1))
    return _records(SPHERE_R * u, -u), np.zeros(len(u), int)


def sphere_irradiance(D, integrator=SCATTER, lamp_in_lights=False):
    """64 points x 4 copies x 512 samples = 131 072; x 1024 at D = 1, where a sample is Le or 0 and 131 072 gave SE 0.478 %; x 2048 at
    D = 2, where the control's red channel is only 2 % away (z -3.4 at 131 072, -7 now).  Measured SE / want on the emulator, largest
    channel: D = 1 0.34 %, D = 2 0.20 %, D = 3 0.39 %, D = 50 0.39 %.
    Power control: the sum with D + 1 terms (a depth test off by one), at D = 1 and D = 2 (q^D shrinks below the noise after that)."""
    items, group = sphere_points()
    control = [integrating_sphere(SPHERE_A, SPHERE_F, SPHERE_LE, D + 1)] if D <= 2 else None
    return Case(f"sphere-irradiance-D{D}-{INTEG_NAME[integrator]}", lambda: sphere_scene(lamp_in_lights), "points",
                {1: 1024, 2: 2048}.get(D, 512), _kw(SPHERE_SEED, D, integrator), [integrating_sphere(SPHERE_A, SPHERE_F, SPHERE_LE, D)],
                items, group, control)


def sphere_camera():
    return camera((0, 0, 1.5), (0, 0, 3), vfov=40.0, aspect=1.0, aperture=0.0)


def sphere_frame(D, flags=0, crowd=False):
    """16 x 16 pixels from between the lamp and the wall, looking away from the lamp: every pixel sees the wall, whose radiance is
    a times what it receives within the D - 1 segments left.  1024 samples per pixel (262 144): measured SE 0.34 % at D = 2, 0.29 % at
    D = 3, 0.28 % at D = 50; D = 1 is exactly 0.  Power control: one segment more, at D = 2 and D = 3."""
    want = np.asarray(SPHERE_A) * integrating_sphere(SPHERE_A, SPHERE_F, SPHERE_LE, D - 1)
    control = np.asarray(SPHERE_A) * integrating_sphere(SPHERE_A, SPHERE_F, SPHERE_LE, D) if 2 <= D <= 3 else None
    tile = lambda v: None if v is None else np.tile(v, (16, 16, 1))
    return Case(f"sphere-frame-D{D}-flags{flags}" + "-crowd" * crowd, lambda: sphere_scene(crowd=crowd), "frame", 1024, _kw(SPHERE_SEED, D, SCATTER), tile(want),
                control=tile(control), cam=sphere_camera(), size=(16, 16), flags=flags)


# ---------------------------------------------------------------- the rectangular light over a Lambertian floor
RECT_A, RECT_LE, RECT = (0.3, 0.6, 0.9), (4.0, 2.0, 1.0), (-0.5, 0.5, -0.75, 0.75)
RECT_H, RECT_SEED, RECT_REPLICAS, TILT_SEED = 1.0, 5, 256, 3
RECT_XZ = ((0.0, 0.0), (0.7, 0.3), (2.0, -1.0))
RECT_VERTS = [(RECT[0], RECT_H, RECT[2]), (RECT[1], RECT_H, RECT[2]), (RECT[1], RECT_H, RECT[3]), (RECT[0], RECT_H, RECT[3])]
TILTED = (((0.2, 0.0, 0.1), (0.3, 1.0, -0.2)), ((1.0, 0.2, 0.5), (-1.0, 1.0, 0.0)))


def rect_scene(lights="bare", floor_y=0.0):
    """the light is FlipFace'd in the world — an xz_rect's outward normal is +y (hittable.rs:230-269), FlipFace turns front_face round
    (hittable.rs:299-311), DiffuseLight emits on the front face only (material.rs:218-225): it shines DOWN — and bare in `lights`, as
    every builder in scene.rs does.  lights: 'bare', 'two' (the bare rect and a dark bare rect elsewhere: Vec::pdf_value averages, Vec::
    random chooses, hittable.rs:420-433), 'flipped' (property B) or 'none'."""
    d = Desc()
    floor = d.xz_rect(-50, 50, -50, 50, floor_y, d.lambertian(*RECT_A))
    light = d.xz_rect(RECT[0], RECT[1], RECT[2], RECT[3], RECT_H, d.light(*RECT_LE))
    world = [floor, d.flip(light)]
    ls = {"bare": [light], "flipped": [d.flip(light)], "none": []}.get(lights)
    if lights == "two":
        dark = d.xz_rect(3, 4, 3, 4, 2.0, d.light(0, 0, 0))
        world.append(d.flip(dark))
        ls = [light, dark]
    return d, d.finish(d.list_(world), ls)


def rect_rays(D, integrator, lights="bare", spp=1024):
    """rays straight down from (x0, 0.5, z0) onto the floor: albedo * Le * F(x0, z0) for any max_depth >= 2.  The floor point's radiance
    is a / pi times its irradiance pi Le F: the scatter integrator samples the cosine (material.rs:85-90) and meets the light's front
    with probability F; the PDF integrator weighs scattering_pdf (material.rs:100-108) by the mixture of the cosine and the light's solid
    angle (main.rs:139-146, util.rs:172-185, Rect::pdf_value / random hittable.rs:271-292).  Nothing else shines and the floor is flat:
    no further bounce adds anything.  256 replicas x 1024 samples.  The scatter estimate at (2, -1) (F = 0.011: SE 1.6 %) is dropped.
    Measured SE / want on the emulator — pdf: 0.15 %, 0.20 %, 0.24 %; scatter: 0.29 %, 0.42 %; two lights: 0.24 %, 0.30 %, 0.38 %.
    Power control: F without the receiver's cosine, int h / (pi r^3) dA (a light pdf that lost its cosine)."""
    xz = RECT_XZ if integrator == PDF else RECT_XZ[:2]
    items, group = _rays([(x, 0.5, z) for x, z in xz], [(0, -1, 0)] * len(xz), RECT_REPLICAS)
    F = np.array([rect_form_factor_parallel(x, z, RECT, RECT_H) for x, z in xz])
    G = np.array([quadrature_parallel(x, z, RECT, RECT_H, m=1000, power=3) for x, z in xz])
    base = np.asarray(RECT_A) * np.asarray(RECT_LE)
    return Case(f"rect-rays-D{D}-{INTEG_NAME[integrator]}-{lights}", lambda: rect_scene(lights), "rays", spp,
                _kw(RECT_SEED, D, integrator), F[:, None] * base, items, group, G[:, None] * base)


def rect_tilted(integrator):
    """irradiance at two tilted receivers under the light, the floor moved down to y = -5: Le * polygon_form_factor.  max_depth 1: the
    first segment alone — the light's front gives Le, anything else 0 — since the floor far below would add its own reflected light to
    the directions under the receivers' horizons, which no closed form gives (measured at max_depth 50: 0.01 % of the value, far below the SE, but not zero).  Both integrators take
    the query's direction and stop there: they agree sample for sample.  256 replicas x 2048 samples (1024 gave 0.48 % at the second
    receiver); measured SE / want 0.23 % and 0.34 %.  Power control: the form factor of the same polygon for the untilted normal (0, 1, 0)."""
    pts, group = _rays([p for p, _ in TILTED], [n for _, n in TILTED], RECT_REPLICAS)
    F = np.array([polygon_form_factor(p, n, RECT_VERTS) for p, n in TILTED])
    G = np.array([polygon_form_factor(p, (0, 1, 0), RECT_VERTS) for p, n in TILTED])
    return Case(f"rect-tilted-{INTEG_NAME[integrator]}", lambda: rect_scene("bare", floor_y=-5.0), "points", 2048,
                _kw(TILT_SEED, 1, integrator), F[:, None] * np.asarray(RECT_LE), pts, group, G[:, None] * np.asarray(RECT_LE))


RECT_CAM = dict(lookfrom=(0.0, 0.9, 0.0), lookat=(0.0, 0.0, 0.0), vup=(0.0, 0.0, 1.0), vfov=20.0, focus=10.0)


def rect_frame_floor_points(w, h, sub=1):
    """where the rays of Camera::get_ray (main.rs:82-94, 111-120; aperture 0) through sub x sub points of every pixel's footprint meet
    the floor, in f64: (h, w, sub, sub, 2) of (x, z).  Pixel (x, y) draws s in [x, x + 1) / (w - 1), t in [y, y + 1) / (h - 1)
    (main.rs:187-188); sub = 1 is the footprint's centre."""
    c = RECT_CAM
    lf, la, vup = (np.asarray(c[k], f64) for k in ("lookfrom", "lookat", "vup"))
    half = math.tan(math.radians(c["vfov"]) / 2.0)
    wv = (lf - la) / np.linalg.norm(lf - la)
    u = np.cross(vup, wv)
    u /= np.linalg.norm(u)
    v = np.cross(wv, u)
    hor, ver = u * (2.0 * half * c["focus"]), v * (2.0 * half * c["focus"])
    llc = lf - hor / 2.0 - ver / 2.0 - wv * c["focus"]
    off = (np.arange(sub) + 0.5) / sub
    s = (np.arange(w)[:, None] + off[None, :]) / (w - 1)                # (w, sub)
    t = (np.arange(h)[:, None] + off[None, :]) / (h - 1)                # (h, sub)
    d = llc + s[None, :, None, :, None] * hor + t[:, None, :, None, None] * ver - lf      # (h, w, sub, sub, 3)
    k = -lf[1] / d[..., 1]
    return np.stack([lf[0] + k * d[..., 0], lf[2] + k * d[..., 2]], -1)


def rect_frame():
    """the floor under the light seen from (0, 0.9, 0) straight down, 16 x 16 pixels, PDF integrator, 256 samples per pixel: the mean
    over pixels of pixel / want(pixel centre) is 1 (measured SE 0.30 %).  footprint_error(): what the centre stands in for."""
    xz = rect_frame_floor_points(16, 16)[:, :, 0, 0]
    F = np.vectorize(lambda x, z: rect_form_factor_parallel(x, z, RECT, RECT_H))(xz[..., 0], xz[..., 1])
    G = np.vectorize(lambda x, z: quadrature_parallel(x, z, RECT, RECT_H, m=400, power=3))(xz[..., 0], xz[..., 1])
    base = np.asarray(RECT_A) * np.asarray(RECT_LE)
    return Case("rect-frame-pdf", rect_scene, "frame", 256, _kw(RECT_SEED, 50, PDF), F[..., None] * base, control=G[..., None] * base,
                cam=camera(**RECT_CAM), size=(16, 16))


def footprint_error(sub=8):
    """largest relative difference, over the 16 x 16 pixels, between F at the footprint's centre and its mean over sub x sub points of the
    footprint (F is smooth: the midpoint rule's own error is far below the difference it measures)"""
    Fv = np.vectorize(lambda x, z: rect_form_factor_parallel(x, z, RECT, RECT_H))
    centre = rect_frame_floor_points(16, 16)[:, :, 0, 0]
    fine = rect_frame_floor_points(16, 16, sub)
    return float(np.abs(Fv(fine[..., 0], fine[..., 1]).mean((2, 3)) / Fv(centre[..., 0], centre[..., 1]) - 1.0).max())


# ---------------------------------------------------------------- the glass ball along its diameter
GLASS_SEED, GLASS_N, GLASS_REPLICAS = 7, 1.5, 256
GLASS_R0 = ((1.0 - GLASS_N) / (1.0 + GLASS_N)) ** 2          # util.rs:26-27: 0.04
GLASS_DEPTHS = (1, 2, 3, 4, 5, 50)
SKY_BACK, SKY_FWD = sky((0, -1, 0)), sky((0, 1, 0))          # (1, 1, 1) and (0.5, 0.7, 1)


def far_dark_light(d):
    """a dark DiffuseLight rect far away, flipped in the world and bare in `lights`: the PDF integrator needs a light"""
    r = d.xz_rect(100, 101, 100, 101, 100.0, d.light(0, 0, 0))
    return d.flip(r), r


def glass_scene():
    d = Desc()
    ball = d.sphere((0, 0, 0), 1.0, d.mat(ffi.VK_MAT_DIELECTRIC, d.solid(1, 1, 1), GLASS_N))
    dark, bare = far_dark_light(d)
    return d, d.finish(d.list_([ball, dark]), [bare])


def glass(D, integrator):
    """Dielectric (material.rs:150-206, both integrators take the same specular branch; main.rs:134-137) on the diameter: P_back (1, 1, 1)
    + P_fwd (0.5, 0.7, 1).  256 replicas x 256 samples = 65 536 (measured SE / want <= 0.11 % for D >= 3); at D = 2 a sample is 1 with
    probability 0.04, sqrt(24 / n): 1.9 % at 65 536, so 256 x 5120 = 1 310 720 two-segment paths, measured 0.43 %.  D = 1 is exactly 0; the blue channel
    of D = 50 is exactly 1.  Power control: the chain one segment longer (D <= 3), or with R0 of index 1.3 (0.017) in place of 0.04."""
    items, group = _rays([(0, -3, 0)], [(0, 1, 0)], GLASS_REPLICAS)
    value = lambda R0, depth: [np.dot(glass_diameter_chain(R0, depth), [SKY_BACK, SKY_FWD])]
    control = None if D == 1 else value(GLASS_R0, D + 1) if D <= 3 else value(((1 - 1.3) / (1 + 1.3)) ** 2, D)
    return Case(f"glass-D{D}-{INTEG_NAME[integrator]}", glass_scene, "rays", 5120 if D == 2 else 256,
                _kw(GLASS_SEED, D, integrator, ffi.VK_BACKGROUND_SKY), value(GLASS_R0, D), items, group, control)


# ---------------------------------------------------------------- a glass pane met at 60 degrees (Schlick off the normal)
PANE_D = (math.sin(math.radians(60.0)), -0.5, 0.0)


def pane_scene():
    d = Desc()
    pane = d.xz_rect(-5, 5, -5, 5, 0.0, d.mat(ffi.VK_MAT_DIELECTRIC, d.solid(1, 1, 1), GLASS_N))
    dark, bare = far_dark_light(d)
    return d, d.finish(d.list_([pane, dark]), [bare])


def pane(integrator):
    """one Dielectric interface (material.rs:150-206) met from its front at cos = 0.5: reflected with probability schlick(0.5, 1 / 1.5)
    = r0 + (1 - r0) 0.5^5 = 0.07 (util.rs:25-29) it sees the sky along reflect(d, n); refracted (util.rs:18-23: Snell, sin' = sin / 1.5)
    it goes on below the pane, where nothing is, and sees the sky along that direction.  The diameter of the ball cannot tell Schlick's
    angular term from none; this can.  256 replicas x 256 samples; measured SE / want 0.035 %.  Power control: r0 alone, 0.04."""
    items, group = _rays([(0, 1, 0)], [PANE_D], GLASS_REPLICAS)
    sin_t = PANE_D[0] / GLASS_N
    refl, refr = sky((PANE_D[0], 0.5, 0.0)), sky((sin_t, -math.sqrt(1.0 - sin_t * sin_t), 0.0))
    value = lambda Rs: [Rs * refl + (1.0 - Rs) * refr]
    return Case(f"pane-{INTEG_NAME[integrator]}", pane_scene, "rays", 256, _kw(GLASS_SEED, 50, integrator, ffi.VK_BACKGROUND_SKY),
                value(GLASS_R0 + (1.0 - GLASS_R0) * 0.5 ** 5), items, group, value(GLASS_R0))


# ---------------------------------------------------------------- a crowd of spheres met on their tops (the rebuilt-tree routes)
TOPS_B, TOPS_R, TOPS_SEED = (0.7, 0.8, 0.9), 0.5, 13
TOPS_GRID = [(2.0 * i, 2.0 * j) for j in range(3) for i in range(6)]


def tops_albedo(k):
    return (0.1 + 0.04 * k, 0.9 - 0.04 * k, 0.3 + 0.02 * k)


def tops_scene():
    """18 Lambertian spheres of radius 0.5, each of its own albedo, centres on the plane y = 0, two units apart; the world a BVH over
    them and nothing in `lights`: a world of spheres only with 16 objects or more, which the lineariser rebuilds by default (exact
    re-treeing) and under VK_SCENE_FAST_ACCEL"""
    d = Desc()
    objs = []
    for k, (x, z) in enumerate(TOPS_GRID):
        c = np.array([x, 0.0, z])
        objs.append((d.sphere(tuple(c), TOPS_R, d.lambertian(*tops_albedo(k))), c - TOPS_R, c + TOPS_R))
    return d, d.finish(_bvh(d, objs)[0], [])


def tops(D, flags=0):
    """a ray straight down onto the top of every sphere: the normal there is +y and no sphere reaches above the tangent plane y = 0.5,
    so every scattered ray (material.rs:85-90) leaves for the solid background B: each sample is albedo_k * B for max_depth >= 2 and 0
    for max_depth 1 (main.rs:126-128, 150-152) — deterministic, SE = 0, the comparison is to f32 rounding (ROUND).  What it pins is
    that every tree view finds sphere k and shades it with ITS material.  256 copies x 4 samples.  Power control: the next sphere's
    albedo."""
    items, group = _rays([(x, 3.0, z) for x, z in TOPS_GRID], [(0, -1, 0)] * len(TOPS_GRID), 256)
    value = lambda shift: [np.asarray(tops_albedo((k + shift) % len(TOPS_GRID))) * np.asarray(TOPS_B) * (D >= 2) for k in range(len(TOPS_GRID))]
    return Case(f"tops-D{D}-flags{flags}", tops_scene, "rays", 4, _kw(TOPS_SEED, D, SCATTER, ffi.VK_BACKGROUND_SOLID, TOPS_B), value(0),
                items, group, value(1) if D >= 2 else None, flags=flags)


# ---------------------------------------------------------------- black fog
FOG_SEED, FOG_DENSITY, FOG_BG, FOG_REPLICAS = 9, 0.7, (0.9, 0.6, 0.3), 256
FOG_DIRS = ((0.0, 1.0, 0.0), (0.6, 0.8, 0.0), (0.0, 3.0, 0.0))
FOG_TOP = 1.5


def fog_scene():
    d = Desc()
    iso = d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(0, 0, 0))
    med = d.medium(d.boxy((-10, 0, -10), (10, FOG_TOP, 10), d.lambertian(1, 1, 1)), FOG_DENSITY, iso)
    dark, bare = far_dark_light(d)
    return d, d.finish(d.big_box(med, dark), [bare])         # (a list may not hold a medium)


def fog(integrator):
    """ConstantMedium (hittable.rs:453-493) with a black Isotropic phase function (material.rs:442-464): the ray from (0, -1, 0) passes
    the slab 0 <= y <= 1.5 unscattered with probability exp(-density * length) — hit_distance = -ln(u) / density (:473) against (rec2.t -
    rec1.t) * |direction| (:471-475) — and then sees the solid background B; scattered, it carries 0.  The third direction is the first
    one three times as long: the same value.  256 replicas x 1024 samples (262 144; at 131 072 the oblique ray gives 0.455 %): measured
    0.27 %, 0.32 %, 0.27 %.  Power controls: see `wrong`."""
    items, group = _rays([(0, -1, 0)] * 3, FOG_DIRS, FOG_REPLICAS)
    length = [FOG_TOP / (d[1] / np.linalg.norm(d)) for d in FOG_DIRS]
    # -density for -1 / density on the first ray; the slab's thickness on the oblique one; the length in units of t on the long one
    wrong = [FOG_TOP / FOG_DENSITY ** 2, FOG_TOP, FOG_TOP / 3.0]
    B = np.asarray(FOG_BG)
    return Case(f"fog-{INTEG_NAME[integrator]}", fog_scene, "rays", 1024, _kw(FOG_SEED, 50, integrator, ffi.VK_BACKGROUND_SOLID, FOG_BG),
                [B * math.exp(-FOG_DENSITY * l) for l in length], items, group, [B * math.exp(-FOG_DENSITY * l) for l in wrong])


# ---------------------------------------------------------------- the mirror (deterministic)
MIRROR_A, MIRROR_O, MIRROR_D = (0.8, 0.6, 0.4), (0.0, 1.0, 0.0), (0.3, -0.7, 0.2)
# largest relative deviation of a sample from the f64 value, measured: emulator 3.68e-8, oracle (through a camera whose ray is the wanted
# one to f32 rounding) 3.68e-8; the bound is 8 x the larger
MIRROR_MEASURED = 3.7e-8
MIRROR_TOL = 8 * MIRROR_MEASURED


def mirror_scene():
    d = Desc()
    m = d.xz_rect(-5, 5, -5, 5, 0.0, d.mat(ffi.VK_MAT_METAL, d.solid(*MIRROR_A), 0.0))
    dark, bare = far_dark_light(d)
    return d, d.finish(d.list_([m, dark]), [bare])


def mirror_want():
    """Metal with fuzz 0 (material.rs:118-141): albedo * sky(reflect(unit(d), n)), reflect: util.rs:14-16"""
    d = np.asarray(MIRROR_D, f64)
    return np.asarray(MIRROR_A) * sky(d - 2.0 * d[1] * np.array([0.0, 1.0, 0.0]))


def mirror(integrator):
    items, group = _rays([MIRROR_O], [MIRROR_D], 64)
    return Case(f"mirror-{INTEG_NAME[integrator]}", mirror_scene, "rays", 4, _kw(1, 50, integrator, ffi.VK_BACKGROUND_SKY), [mirror_want()],
                items, group)


def mirror_deviation(values):
    """largest relative deviation of (.., >= 3) samples or means from the f64 value"""
    v = np.asarray(values, f64)[..., :3].reshape(-1, 3)
    return float(np.abs(v / mirror_want() - 1.0).max())


# ---------------------------------------------------------------- what the closed forms cannot pin ("Closed-form radiometry")
def property_a():
    """A sphere in `lights` biases the PDF integrator.  random_to_sphere (hittable.rs:123-134) scales x and y by 1 - z^2, not by its
    root: the directions stay inside the cone but are not uniform over it, while Sphere::pdf_value (hittable.rs:104-113) says they are.
    The integrating sphere with the lamp in `lights`, PDF integrator, depth 50, sits +0.5 % / +1.1 % / +2.1 % above the radiometric
    value (measured here: +1.0 % / +1.7 % / +2.7 %, z 2.7 / 7.2 / 8.3 at 131 072 samples).  That is the reference's own; the library must keep reproducing it: the case's `want` is the
    radiometric value and the test asserts that blue DIFFERS from it by |z| > 4."""
    return sphere_irradiance(50, PDF, lamp_in_lights=True)


def property_b():
    """A FlipFace'd entry in `lights` falls back to the trait defaults: pdf_value 0 and random (1, 0, 0) (hittable.rs:36-41; FlipFace
    forwards hit and bounding_box only, :299-311).  The light half of the mixture then draws (1, 0, 0), along the floor: cos = 0,
    pdf = 0, scattering_pdf = 0: 0 / 0, a NaN sample, dropped (main.rs:192-196).  The cosine half alone has pdf = cos / (2 pi): twice the
    value, half the time.  So half of the samples are NaN, the mean still meets the closed form, at twice the variance.  The ray at
    (0, 0): 256 replicas x 2048 samples, SE 0.32 % (1024: 0.454 %, with 130 790 of 262 144 samples dropped and z = 1.06)."""
    c = rect_rays(50, PDF, "flipped", spp=2048)
    keep = c.group == 0
    c.items, c.group, c.want, c.control = c.items[keep], c.group[keep], c.want[:1], c.control[:1]
    return c


# ---------------------------------------------------------------- the list the two test modules run
def _statistical():
    yield from ((f"sphere-irradiance-D{D}", lambda D=D: sphere_irradiance(D)) for D in SPHERE_DEPTHS)
    yield from ((f"sphere-frame-D{D}", lambda D=D: sphere_frame(D)) for D in SPHERE_DEPTHS)
    yield "sphere-frame-D3-reference-tree", lambda: sphere_frame(3, ffi.VK_SCENE_REFERENCE_TREE)
    yield "sphere-frame-D3-fast-accel", lambda: sphere_frame(3, ffi.VK_SCENE_FAST_ACCEL)
    yield "sphere-crowd-frame-D3", lambda: sphere_frame(3, 0, crowd=True)
    yield "sphere-crowd-frame-D3-reference-tree", lambda: sphere_frame(3, ffi.VK_SCENE_REFERENCE_TREE, crowd=True)
    yield "sphere-crowd-frame-D3-fast-accel", lambda: sphere_frame(3, ffi.VK_SCENE_FAST_ACCEL, crowd=True)
    for integ in (PDF, SCATTER):
        yield from ((f"rect-rays-D{D}-{INTEG_NAME[integ]}", lambda D=D, integ=integ: rect_rays(D, integ)) for D in (2, 50))
    yield "rect-rays-two-lights", lambda: rect_rays(50, PDF, "two")
    yield from ((f"rect-tilted-{INTEG_NAME[integ]}", lambda integ=integ: rect_tilted(integ)) for integ in (PDF, SCATTER))
    yield "rect-frame", rect_frame
    for integ in (PDF, SCATTER):
        yield from ((f"glass-D{D}-{INTEG_NAME[integ]}", lambda D=D, integ=integ: glass(D, integ)) for D in GLASS_DEPTHS)
    yield from ((f"pane-{INTEG_NAME[integ]}", lambda integ=integ: pane(integ)) for integ in (PDF, SCATTER))
    yield from ((f"fog-{INTEG_NAME[integ]}", lambda integ=integ: fog(integ)) for integ in (PDF, SCATTER))
    yield from ((f"tops-D{D}", lambda D=D: tops(D)) for D in (1, 2, 50))
    yield "tops-D50-reference-tree", lambda: tops(50, ffi.VK_SCENE_REFERENCE_TREE)
    yield "tops-D50-fast-accel", lambda: tops(50, ffi.VK_SCENE_FAST_ACCEL)


STATISTICAL = dict(_statistical())          # name -> a function that builds the Case
