"""The lens, the shutter and what they blur, in plain f64 numpy.  TESTS ONLY; shared by tests/test_camera_laws.py (oracle, emulators) and
tests/test_gpu_camera_laws.py (the public calls on the device).

Everything here is written from the reference's own lines (main.rs:111-120 Camera::get_ray, main.rs:187-189 the pixel loop,
util.rs:41-50 random_in_unit_disk, hittable.rs:147-150 MovingSphere::center, rand 0.7.3 UniformFloat::sample_single), cited beside each
function.  It imports geometry_ref for Camera::new, the focus point, lens coordinates, pixel_st and the f64 closest hit, and nothing of the
oracle, of an emulator or of another *_ref.py; no formula is taken from vk_trace.h or oracle.cpp.  The RNG stream and rand's two float mappings (gen::<f32>() and gen_range's value in
[1, 2) minus 1) come in through oracle_ffi.draws, passed by the caller; tests/test_math_rng.py pins them.

Stability (properties of the f64 values alone):
  a rejection test x^2 + y^2 < 1 within 2^-22 of 1 (the f32 sum of two rounded squares may fall on the other side);
  a time within BOUND_TIME of time1 (the f32 value may round to time1, which gen_range redraws: `if res < high`).
Such samples are excluded and counted; at most MAX_EXCLUDED of a frame's."""
import math

import numpy as np

import geometry_ref as G
from vecchio_amd import ffi               # the constant that names a DiffuseLight in a description, nothing else

f64 = np.float64
N_DRAWS = 48                       # draws read per stream: 2 + 2 * pairs + 1; 22 rejected pairs in a row have probability 0.215^22
MAX_EXCLUDED = 0.01

# Lens coordinates, relative to the focus distance: 4 x the ORACLE's worst deviation from the f64 value over every camera, frame and
# first sample of tests/test_camera_laws.py part 1, measured on the CPU (pytest -s prints it per camera; DESIGN.md holds the table).
# Nothing from the emulator or the device.  The z, SE and counts below are what the same module prints for the oracle's data; only `lens`
# and `rejected_share` are read by a test (test_the_measured_record_is_the_oracle_s), the rest is the record DESIGN.md quotes.
MEASURED = dict(
    lens=6.76e-8,                  # aperture 2.0 (R = 1, focus 4.5): the f32 sum origin + offset, an ulp of 4 < lookfrom.z + offset < 8 is 4.8e-7
    #                                (the twelve cameras of test_geometry at aperture 0.3: 5.89e-8; the rolled one and the short shutter: 5.97e-8)
    time=5.96e-8,                  # the oracle's worst time deviation, shutter (0.25, 1.75): bound 2^-23 * 1.75 = 2.09e-7; (0.25, 0.2501): 1.49e-8
    rejected_share=0.2239,         # share of part 1's 5392 samples per camera that rejected one or more pairs (uniform draws: 1 - pi / 4 = 0.2146)
    # part 2, 65 536 samples of seed 11 (the draws, hence the z, are the same for the three cameras; the time's scale is the shutter's)
    laws=dict(statistics=37, worst_z=3.02, worst="corr jitter y, right-hand pixel's", repeated=0, E_r2=(0.49734, 0.00113), E_time_01=(0.49900, 0.00113),
              E_time_long=(0.99850, 0.00169), control_z={"uniform in radius": 145.7, "the square": -150.4, "R = aperture": -1334.6, "shutter [0, 1)": 294.2}),
    # part 3, the oracle's counts (the emulator's are the same, and so are the f64 simulation's, sample for sample):
    #   name: (partial cells, chi-square, pooled z, worst single |z|, pooled z of the controls)
    edge={"vertical-D2": (23, 38.9, 2.34, 2.65, {"uniform in radius": 740.4, "R = aperture": 3238.6}),
          "vertical-D8": (12, 12.8, 0.17, 2.13, {"uniform in radius": 552.9, "R = aperture": 2335.1}),
          "horizontal-D2": (23, 23.1, 0.01, 2.52, {"uniform in radius": 812.6, "R = aperture": 3167.2}),
          "horizontal-D8": (12, 5.6, -1.31, 1.51, {"uniform in radius": 539.1, "R = aperture": 2349.5})},
    quadrature=dict(against_segment_formula=(6.42e-4, 6.01e-4), sphere_self=5.1e-4, sphere_tenth_of_se=2.05e-3, moving_pinhole_over_se=0.057,
                    moving_lens_self=8.59e-4, moving_lens_tenth_of_se=9.79e-4, five_d_midpoints=5.54e-3),
    sphere=(39, 41.7, 0.31, 2.64),
    motion_blur=(91, 73.1, -1.33, 2.36, {"centre clamped": 3774.5, "camera shutter [0, 1)": 481787.6, "interpolated over the camera's shutter": 42053.7}),
    motion_blur_through_a_lens=(81, 83.0, 0.16, 2.36),
    #   cloud under aperture 0.6: (share of samples that name a sphere, unstable share, share of winners that differ from the pinhole's)
    clouds=dict(layer=(0.663, 0.000326, 0.033), shared=(0.539, 0.000326, 0.162), inside=(0.567, 0.000326, 0.412), grid=(0.658, 0.000977, 0.095)),
)
BOUND_LENS = 4.0 * MEASURED["lens"]


def bound_time(time0, time1):
    """two rounded f32 operations on the draw (v * scale, + low; the scale time1 - time0 is exact for the shutters used): 2 half-ulps of
    at most max(|time0|, |time1|)"""
    return 2.0 ** -23 * max(abs(time0), abs(time1))


# ================================================================ 1. values
def stream_samples(draws, seed, width, height, first_sample, n_samples, window=None):
    """get_ray's consumption of every sample's stream (seed, pixel = y width + x, sample), main.rs:182-189 and :111-120: draws 0 and 1
    are the jitter (main.rs:187-188, gen::<f32>()); from draw 2 on pairs go through gen_range(-1, 1) until x^2 + y^2 < 1
    (util.rs:43-49: `if p.length2() >= 1.0 { continue }`), whatever the lens radius (main.rs:113 calls random_in_unit_disk before it
    multiplies); the next draw is the time's (main.rs:118).  window: (x0, y0, w, h) of the frame, default all of it.
    Returns a dict of (h, w, n) arrays: xi (.., 2), disc (.., 2) the accepted pair, v01 the time's draw in [0, 1), rejected (pairs
    rejected), near (a rejection test within 2^-22 of 1)."""
    x0, y0, w, h = window or (0, 0, width, height)
    n = h * w * n_samples
    u01, pm1 = np.zeros((n, N_DRAWS)), np.zeros((n, N_DRAWS))
    i = 0
    for y in range(y0, y0 + h):
        for x in range(x0, x0 + w):
            for k in range(first_sample, first_sample + n_samples):
                u01[i] = draws(seed, y * width + x, k, 0, N_DRAWS)
                pm1[i] = draws(seed, y * width + x, k, 1, N_DRAWS, -1.0, 1.0)
                i += 1
    done, rejected, near = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, bool)
    disc, v01 = np.zeros((n, 2)), np.zeros(n)
    for j in range(2, N_DRAWS - 2, 2):
        x, y = pm1[:, j], pm1[:, j + 1]
        l2 = x * x + y * y
        near |= ~done & (np.abs(l2 - 1.0) < 2.0 ** -22)
        take = ~done & (l2 < 1.0)
        disc[take] = np.stack([x, y], 1)[take]
        v01[take] = (pm1[take, j + 2] + 1.0) / 2.0     # gen_range(-1, 1) = 2 v - 1 exactly (vk_math.h gen_pm1's note): v is the draw in [0, 1)
        rejected += ~done & ~take
        done |= take
    assert done.all(), "a stream that rejects more pairs than N_DRAWS holds"
    shape = (h, w, n_samples)
    return dict(xi=u01[:, :2].reshape(shape + (2,)), disc=disc.reshape(shape + (2,)), v01=v01.reshape(shape), rejected=rejected.reshape(shape),
                near=near.reshape(shape), window=(x0, y0, w, h), frame=(width, height))


def get_ray(cam, st):
    """Camera::get_ray, main.rs:111-120, for stream_samples()' samples: (origin, direction, time, unstable).  rd = disc * lens_radius;
    offset = u rd.x + v rd.y; origin + offset; lower_left + s horizontal + t vertical - origin - offset; gen_range(time0, time1) =
    v * (time1 - time0) + time0 (UniformFloat::sample_single, redrawn while >= time1)."""
    x0, y0, w, h = st["window"]
    width, height = st["frame"]
    y, x = np.mgrid[y0:y0 + h, x0:x0 + w]
    s, t = G.pixel_st(st["xi"], x[..., None], y[..., None], width, height)
    rd = st["disc"] * cam["lens_radius"]
    offset = rd[..., 0:1] * cam["u"] + rd[..., 1:2] * cam["v"]
    origin = cam["origin"] + offset
    direction = G.focus_point(cam, s, t) - origin
    time = cam["time0"] + st["v01"] * (cam["time1"] - cam["time0"])
    unstable = st["near"] | (cam["time1"] - time <= bound_time(cam["time0"], cam["time1"]))
    return origin, direction, time, unstable


def deviations(cam, focus, st, origin, time, what):
    """an f32 evaluation's origins and times (h, w, n, ...) against get_ray's: (worst lens deviation relative to the focus distance,
    worst time deviation, excluded share).  The excluded share is capped here."""
    want_o, _, want_t, unstable = get_ray(cam, st)
    ok = ~unstable
    assert unstable.mean() <= MAX_EXCLUDED, f"{what}: {unstable.mean():.4f} of the samples are unstable"
    a, b, c = G.lens_coordinates(cam, np.asarray(origin, f64))
    wa, wb, _ = G.lens_coordinates(cam, want_o)
    lens = float(np.maximum(np.maximum(np.abs(a - wa), np.abs(b - wb)), np.abs(c))[ok].max()) / focus
    return lens, float(np.abs(np.asarray(time, f64) - want_t)[ok].max()), float(unstable.mean())


# ================================================================ 2. laws
def _z_mean(x, want):
    x = np.asarray(x, f64).reshape(-1)
    se = x.std(ddof=1) / math.sqrt(x.size)
    return dict(got=float(x.mean()), want=float(want), se=float(se), z=float((x.mean() - want) / se))


def _z_share(sel, p):
    sel = np.asarray(sel).reshape(-1)
    se = math.sqrt(p * (1.0 - p) / sel.size)
    return dict(got=float(sel.mean()), want=float(p), se=se, z=float((sel.mean() - p) / se))


def _z_corr(x, y):
    """the mean of the product of the two standardised samples against 0, its SE from the products"""
    x, y = np.asarray(x, f64).reshape(-1), np.asarray(y, f64).reshape(-1)
    return _z_mean((x - x.mean()) / x.std() * (y - y.mean()) / y.std(), 0.0)


def statistics(xi, a, b, time, time0, time1):
    """name -> dict(got, want, se, z) of everything the issue holds.  xi (h, w, n, 2): the jitter (part 1's draws); a, b (h, w, n): the
    lens coordinates over the lens RADIUS (None at aperture 0); time (h, w, n).  The disc: uniform over the unit disc (util.rs:41-50),
    E a = E b = E ab = 0, E a^2 = E b^2 = 1/4, E r^2 = int_0^1 r^2 2r dr = 1/2, E r^4 = 1/3, P(r < 1/2) = 1/4.  The time: uniform over
    [time0, time1) (main.rs:118)."""
    out = {}
    series = {"jitter x": xi[..., 0], "jitter y": xi[..., 1], "time": time}
    if a is not None:
        r2 = a * a + b * b
        out["E a"], out["E b"] = _z_mean(a, 0.0), _z_mean(b, 0.0)
        out["E a^2"], out["E b^2"], out["E ab"] = _z_mean(a * a, 0.25), _z_mean(b * b, 0.25), _z_mean(a * b, 0.0)
        out["E r^2"], out["E r^4"] = _z_mean(r2, 0.5), _z_mean(r2 * r2, 1.0 / 3.0)
        out["P r < 1/2"] = _z_share(r2 < 0.25, 0.25)
        for name, sel in (("++", (a >= 0) & (b >= 0)), ("-+", (a < 0) & (b >= 0)), ("--", (a < 0) & (b < 0)), ("+-", (a >= 0) & (b < 0))):
            out[f"quadrant {name}"] = _z_share(sel, 0.25)
        series.update({"lens a": a, "lens b": b})
    mid, span = (time0 + time1) / 2.0, time1 - time0
    out["E time"] = _z_mean(time, mid)
    out["Var time"] = _z_mean((time - mid) ** 2, span * span / 12.0)
    for q in range(4):
        out[f"shutter quarter {q}"] = _z_share((time >= time0 + q * span / 4.0) & (time < time0 + (q + 1) * span / 4.0), 0.25)
    names = sorted(series)
    group = lambda k: k.split()[0]
    for i, p in enumerate(names):
        for q in names[i + 1:]:
            if group(p) != group(q) or group(p) == "jitter":
                out[f"corr {p}, {q}"] = _z_corr(series[p], series[q])
    for k in names:
        out[f"corr {k}, right-hand pixel's"] = _z_corr(series[k][:, :-1], series[k][:, 1:])
        out[f"corr {k}, successor's"] = _z_corr(series[k][:, :, :-1], series[k][:, :, 1:])
    return out


def controls(a, b, time, aperture, time0, time1):
    """name -> z of the misreadings the same data must reject by |z| > 8: a disc uniform in radius (E r^2 = int_0^1 r^2 dr = 1/3), the
    square (E x^2 + y^2 = 2/3), R = aperture (the coordinates over the aperture have E r^2 = 1/2 only if the radius were the aperture),
    a shutter of [0, 1) (where the camera's is another)."""
    out = {}
    if a is not None:
        r2 = a * a + b * b
        out["uniform in radius"] = _z_mean(r2, 1.0 / 3.0)["z"]
        out["the square"] = _z_mean(r2, 2.0 / 3.0)["z"]
        out["R = aperture"] = _z_mean(r2 / 4.0, 0.5)["z"]         # a, b are over aperture / 2
    if (time0, time1) != (0.0, 1.0):
        out["shutter [0, 1)"] = _z_mean(time, 0.5)["z"]
    return out


# ================================================================ 3. frames
def segment_share(q):
    """the share of the unit disc with abscissa >= q: (acos q - q sqrt(1 - q^2)) / pi, 1 below -1, 0 above 1"""
    q = np.clip(np.asarray(q, f64), -1.0, 1.0)
    return (np.arccos(q) - q * np.sqrt(1.0 - q * q)) / math.pi


def radius_uniform_share(q, m=2048):
    """the control: P(r cos(phi) >= q) for r uniform in [0, 1), phi uniform: int_0^1 acos(clip(q / r)) / pi dr, by midpoints"""
    q = np.asarray(q, f64)
    r = (np.arange(m) + 0.5) / m
    return (np.arccos(np.clip(q[..., None] / r, -1.0, 1.0)) / math.pi).mean(-1)


def edge_coverage(cam, focus, depth, edge, axis, n_pixels, share=segment_share, radius=None, m=4096):
    """The coverage of each column (axis 0: the emitter covers x >= edge) or row (axis 1: y >= edge) of a frame by an emitter at
    z = -depth, for a camera at the origin looking down -z with u = +x, v = +y.  A sample with focus-plane abscissa X_f and lens abscissa
    a meets the plane at a (1 - D / F) + X_f D / F (main.rs:115-117: the ray runs from origin + offset to the focus point, reached at
    parameter 1, the plane at parameter D / F).  So it is covered where a * k >= edge - X_f D / F, k = 1 - D / F: the unit disc's segment
    share at q = (edge - X_f D / F) / (k R) for k > 0, its complement for k < 0; averaged over the pixel's jitter by m midpoints.
    Returns (p, exact): exact = 0 or 1 where the law puts the whole pixel there (both ends of the jitter, p being monotone), else -1."""
    R = cam["lens_radius"] if radius is None else radius
    k = 1.0 - depth / focus
    vec = cam["horizontal"] if axis == 0 else cam["vertical"]
    lo = cam["lower_left_corner"][axis]

    def p_at(jitter):
        s = (np.arange(n_pixels)[:, None] + jitter) / (n_pixels - 1)             # main.rs:187-188
        xf = lo + s * vec[axis]
        q = (edge - xf * depth / focus) / (k * R)
        return share(q) if k > 0 else 1.0 - share(q)
    p = p_at((np.arange(m) + 0.5) / m).mean(1)
    ends = np.concatenate([p_at(np.array([0.0])), p_at(np.array([1.0]))], 1)
    exact = np.where((ends == 0.0).all(1), 0, np.where((ends == 1.0).all(1), 1, -1))
    return p, exact


def lens_grid(ml):
    """(n, 2): the midpoints of the ml x ml square strata of [-1, 1)^2 that lie in the unit disc (the reference's own rejection,
    util.rs:41-50), the grid turned by 0.6 rad: a polar grid is aligned with the rim of a centred sphere's image and errs by a whole ring
    there, an upright one with an upright edge and errs by a whole row"""
    g = (np.arange(ml) + 0.5) / ml * 2.0 - 1.0
    gx, gy = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    inside = gx * gx + gy * gy < 1.0
    cs, sn = math.cos(0.6), math.sin(0.6)
    return np.stack([cs * gx - sn * gy, sn * gx + cs * gy], 1)[inside]


def shutter_share(o, d, c0, c1, s0, s1, radius, T0, T1, clamp=False):
    """The share of the camera's shutter [T0, T1) (main.rs:118: uniform) during which the ray o + t d meets a MovingSphere: its centre
    at time t is c0 + (c1 - c0) (t - s0) / (s1 - s0) (hittable.rs:147-150, no clamp); the ray meets the sphere where the centre's
    distance from the ray's line is below the radius: with e = d / |d| and w(t) = c(t) - o - ((c(t) - o) . e) e = w0 + w1 t, |w|^2 < r^2
    is a quadratic in t, and the share is the part of the shutter inside its roots.  clamp (a control): the centre stands still outside
    (s0, s1).  The sphere has to be in front of every ray that could meet it."""
    c0, c1 = np.asarray(c0, f64), np.asarray(c1, f64)
    vel = (c1 - c0) / (s1 - s0)
    base = c0 - vel * s0 - o                                                      # c(t) - o = base + vel t
    e = d / np.linalg.norm(d, axis=-1, keepdims=True)
    along0, along1 = (base * e).sum(-1), (vel * e).sum(-1)
    w0, w1 = base - along0[..., None] * e, vel - along1[..., None] * e
    A, B, Cc = (w1 * w1).sum(-1), (w0 * w1).sum(-1), (w0 * w0).sum(-1) - radius * radius
    disc = B * B - A * Cc
    root = np.sqrt(np.maximum(disc, 0.0))
    ta, tb = (-B - root) / A, (-B + root) / A
    for t in (min(T0, s0), max(T1, s1)):
        assert ((along0 + along1 * t)[disc > 0] > radius).all(), "the sphere is not in front"
    inside = lambda lo, hi: np.where(disc > 0, np.maximum(np.minimum(tb, hi) - np.maximum(ta, lo), 0.0), 0.0)
    if clamp:
        length = inside(max(T0, s0), min(T1, s1)) + np.where((disc > 0) & (ta < s0) & (s0 < tb), max(s0 - T0, 0.0), 0.0) \
            + np.where((disc > 0) & (ta < s1) & (s1 < tb), max(T1 - s1, 0.0), 0.0)
    else:
        length = inside(T0, T1)
    return length / (T1 - T0)


def moving_coverage(cam, width, height, c0, c1, s0, s1, radius, shutter=None, clamp=False, over_camera=False, m=24, ml=0, rows=None):
    """The coverage of every pixel (height, width) by a MovingSphere: shutter_share() of the f64 ray of get_ray's form (main.rs:111-120),
    averaged over the jitter by m x m midpoints and, where ml > 0, over the lens by lens_grid(ml) (ml = 0: a pinhole).  The time is
    integrated exactly, so what remains to the midpoints is continuous.  The controls: shutter = (0, 1); clamp; over_camera: the
    interpolation runs over the camera's shutter instead of the sphere's.  rows: only these rows of the frame (the others stay 0)."""
    T0, T1 = shutter or (cam["time0"], cam["time1"])
    if over_camera:
        s0, s1 = cam["time0"], cam["time1"]
    j = (np.arange(m) + 0.5) / m
    lens = lens_grid(ml) * cam["lens_radius"] if ml else np.zeros((1, 2))
    offset = lens[:, 0:1] * cam["u"] + lens[:, 1:2] * cam["v"]
    out = np.zeros((height, width))
    for y in (range(height) if rows is None else rows):
        x, jy, jx = np.meshgrid(np.arange(width), j, j, indexing="ij")
        focus = G.focus_point(cam, (x + jx) / (width - 1), (y + jy) / (height - 1))[..., None, :]
        o = cam["origin"] + offset
        out[y] = shutter_share(o, focus - o, c0, c1, s0, s1, radius, T0, T1, clamp).mean((1, 2, 3))
    return out


def pooled(k, n, p, partial):
    """(chi-square over the partial cells, its degrees of freedom m, z = (chi2 - m) / sqrt(2 m), the worst single |z|)"""
    k, p = np.asarray(k, f64)[partial], np.asarray(p, f64)[partial]
    z = (k - n * p) / np.sqrt(n * p * (1.0 - p))
    m = int(partial.sum())
    chi2 = float((z * z).sum())
    return chi2, m, (chi2 - m) / math.sqrt(2.0 * m), float(np.abs(z).max())


def lit(sc, hit):
    """the rays that see light at max_depth 1: the first hit is the front face of a DiffuseLight (material.rs DiffuseLight::emitted:
    `if rec.front_face`; every other material emits nothing)"""
    kinds = np.array([m[0] for m in sc.materials])
    return hit["hit"] & hit["front"] & (kinds[hit["material"]] == ffi.VK_MAT_DIFFUSE_LIGHT)


def simulate_counts(draws, cam, sc, seed, width, height, spp, rows=4):
    """the f64 frame: per pixel, how many of its spp samples' f64 rays (get_ray) meet an emitter's front face first (closest_hit;
    DiffuseLight emits on the front face only, material.rs emitted) — (counts (height, width), unstable share).  Walked `rows` rows at
    a time."""
    counts, unstable = np.zeros((height, width), np.int64), 0
    for y0 in range(0, height, rows):
        h = min(rows, height - y0)
        st = stream_samples(draws, seed, width, height, 0, spp, (0, y0, width, h))
        o, d, t, bad = get_ray(cam, st)
        hit, record = G.closest_hit(sc, o.reshape(-1, 3), d.reshape(-1, 3), t.reshape(-1))
        seen = lit(sc, hit)
        unstable += int((bad.reshape(-1) | ~G.stable(record)).sum())
        counts[y0:y0 + h] = seen.reshape(h, width, spp).sum(2)
    return counts, unstable / (width * height * spp)
