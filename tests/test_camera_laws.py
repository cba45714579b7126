"""The lens, the shutter and what they blur, on the CPU: the oracle and the emulators against tests/camera_laws_ref.py, f64 laws written
from the reference's lines alone.  Every other camera test holds the oracle and vk_trace.h start_sample_core to each other or to ranges;
a misreading the two share (a time drawn before the lens, no lens draw at aperture 0, rd.y on u, a disc uniform in radius, a shutter of
[0, 1), a clamped MovingSphere) passes them and fails here.  tests/test_gpu_camera_laws.py runs the same cases through the public calls
on the device.

1. values: every sample's lens point and time from its stream's draws;  2. laws: what the draws add up to;  3. frames: a defocused edge,
a defocused sphere, sphere clouds under a lens, motion blur and both together, as counts of samples that see an emitter.

Run with -s for the oracle's deviations (what camera_laws_ref.MEASURED holds) and every z."""
import math

import numpy as np
import pytest

import camera_laws_ref as L
import geometry_ref as G
import test_geometry as T
from descs import Desc, camera, params
from test_splat_laws import ROLLED
from vecchio_amd import ffi

f32, f64 = np.float32, np.float64
SEED, SEED2 = 11, 0x5EED2
LE = (1.0, 0.5, 2.0)               # exact in f32: a frame's mean times N is a count


# ================================================================ cameras
def camera_pair(c):
    """(the library's camera, the f64 camera): aperture and shutter of the f64 one are the f32 values the description holds"""
    cam = camera(c["lookfrom"], c["lookat"], c["vfov"], c["aspect"], c["aperture"], c["focus"], c["t0"], c["t1"], c["vup"])
    c64 = G.camera_new(c["lookfrom"], c["lookat"], c["vup"], c["vfov"], c["aspect"], float(f32(c["aperture"])), c["focus"],
                       float(f32(c["t0"])), float(f32(c["t1"])))
    return cam, c64


WIDE = dict(ROLLED, aperture=2.0)
SHORT = dict(ROLLED, t0=0.25, t1=0.2501)
LONG = dict(ROLLED, t0=0.25, t1=1.75)
VALUE_CAMERAS = [("rolled", ROLLED)] + [(T.camera_id(c), c) for c in T.CAMERAS] + [("aperture2", WIDE), ("shutter0.25-0.2501", SHORT)]
VALUE_FRAMES = ((21, 13), (8, 8))
VALUE_SPP, VALUE_FIRSTS = 8, (0, 5)
_streams = {}


def streams(oracle, seed, width, height, first, n, window=None):
    key = (seed, width, height, first, n, window)
    if key not in _streams:
        _streams[key] = L.stream_samples(oracle.draws, seed, width, height, first, n, window)
    return _streams[key]


def far_sphere():
    d = Desc()
    s = d.sphere((0, 0, -100), 1.0, d.lambertian(0.5, 0.5, 0.5))
    return d, d.finish(d.big_box(s, s))


def in_id_order(rays, shape):
    return rays["origin"].reshape(shape + (3,)), rays["direction"].reshape(shape + (3,)), rays["time"].reshape(shape)


def hold_values(c, c64, st, origin, direction, time, what):
    """an f32 evaluation of a window's samples against get_ray's values: the deviations"""
    lens, dt, excluded = L.deviations(c64, c["focus"], st, origin, time, what)
    assert lens <= L.BOUND_LENS, f"{what}: a lens point deviates by {lens:.3g} of the focus distance, bound {L.BOUND_LENS:.3g}"
    bound = L.bound_time(c64["time0"], c64["time1"])
    assert dt <= bound, f"{what}: a time deviates by {dt:.3g}, bound {bound:.3g}"
    if c["aperture"] == 0.0:
        assert (np.asarray(origin) == f32(c["lookfrom"])).all(), what
    return lens, dt, excluded


# ================================================================ 1. values
@pytest.mark.parametrize("name,c", VALUE_CAMERAS, ids=[n for n, _ in VALUE_CAMERAS])
def test_values(name, c, oracle, built):
    import emu_film_ffi
    d, desc = far_sphere()
    cam, c64 = camera_pair(c)
    worst, rejected, total = [0.0, 0.0, 0.0, 0.0], 0, 0
    for width, height in VALUE_FRAMES:
        for first in VALUE_FIRSTS:
            p = params(width, height, first + VALUE_SPP, seed=SEED, integrator=ffi.VK_INTEGRATOR_SCATTER)     # a film's windows end at its samples
            st = streams(oracle, SEED, width, height, first, VALUE_SPP)
            rejected, total = rejected + int((st["rejected"] > 0).sum()), total + st["rejected"].size
            fh = oracle.first_hits(desc, cam, p, first, VALUE_SPP)
            lens, dt, _ = hold_values(c, c64, st, fh["origin"], fh["direction"], fh["time"], f"oracle {name} {width}x{height} from {first}")
            rays, _ = emu_film_ffi.emit(cam, p, 0, 0, width, height, first, VALUE_SPP)
            le, de, _ = hold_values(c, c64, st, *in_id_order(rays, (height, width, VALUE_SPP)), f"emulator {name} {width}x{height} from {first}")
            worst = [max(a, b) for a, b in zip(worst, (lens, dt, le, de))]
    share = rejected / total
    print(f"\n   {name}: oracle - f64: lens {worst[0]:.3g} of the focus distance, time {worst[1]:.3g}; emulator: {worst[2]:.3g}, {worst[3]:.3g}; "
          f"{share:.4f} of {total} samples rejected a pair")
    assert share >= 0.15, f"only {share:.3f} of the samples rejected a pair: the loop's draw count is not exercised"


def test_the_measured_record_is_the_oracle_s(oracle, built):
    """camera_laws_ref.MEASURED['lens'] is the oracle's worst deviation over part 1's cameras (the bound is 4 x it), to its three digits"""
    d, desc = far_sphere()
    worst, rejected, total = 0.0, 0, 0
    for name, c in VALUE_CAMERAS:
        cam, c64 = camera_pair(c)
        for width, height in VALUE_FRAMES:
            for first in VALUE_FIRSTS:
                p = params(width, height, VALUE_SPP, seed=SEED, integrator=ffi.VK_INTEGRATOR_SCATTER)
                st = streams(oracle, SEED, width, height, first, VALUE_SPP)
                fh = oracle.first_hits(desc, cam, p, first, VALUE_SPP)
                worst = max(worst, L.deviations(c64, c["focus"], st, fh["origin"], fh["time"], name)[0])
                rejected, total = rejected + int((st["rejected"] > 0).sum()), total + st["rejected"].size
    print(f"\n   oracle lens deviation over all cameras {worst:.4g}; rejected share {rejected / total:.4f}")
    assert abs(worst / L.MEASURED["lens"] - 1.0) < 0.01, worst
    assert abs(rejected / total - L.MEASURED["rejected_share"]) < 5e-4


# ================================================================ 2. laws
LAW_W, LAW_H, LAW_SPP = 64, 32, 32
LAW_CAMERAS = [("rolled", ROLLED), ("aperture2", WIDE), ("shutter0.25-1.75", LONG)]


def law_data(oracle, c, c64, seed, spp, origin, time):
    """(xi, a / R, b / R, time) of a route's origins and times (h, w, n, ...)"""
    xi = streams(oracle, seed, LAW_W, LAW_H, 0, spp)["xi"]
    a, b, _ = G.lens_coordinates(c64, np.asarray(origin, f64))
    R = c64["lens_radius"]
    return xi, a / R, b / R, np.asarray(time, f64)


def hold_laws(route, oracle, c, what, record=None):
    """route(seed, spp) -> (origin, time) of the 64 x 32 frame.  Every statistic within 4 SE; a failing one is repeated once at 4 N with
    a second seed; the controls rejected by |z| > 8."""
    _, c64 = camera_pair(c)
    xi, a, b, time = law_data(oracle, c, c64, SEED, LAW_SPP, *route(SEED, LAW_SPP))
    stats = L.statistics(xi, a, b, time, c64["time0"], c64["time1"])
    failing = [k for k, s in stats.items() if abs(s["z"]) > 4.0]
    if record is not None:
        record.update(stats)
    if failing:
        again = L.statistics(*law_data(oracle, c, c64, SEED2, 4 * LAW_SPP, *route(SEED2, 4 * LAW_SPP)), c64["time0"], c64["time1"])
        for k in failing:
            assert abs(again[k]["z"]) <= 4.0, f"{what}: {k}: {stats[k]} at N, {again[k]} at 4 N"
    ctl = L.controls(a, b, time, c["aperture"], c64["time0"], c64["time1"])
    for k, z in ctl.items():
        assert abs(z) > 8.0, f"{what}: the control '{k}' is not rejected: z = {z:.2f}"
    return stats, ctl, failing


@pytest.mark.parametrize("name,c", LAW_CAMERAS, ids=[n for n, _ in LAW_CAMERAS])
def test_laws(name, c, oracle, built):
    import emu_film_ffi
    d, desc = far_sphere()
    cam, _ = camera_pair(c)

    def by_oracle(seed, spp):
        fh = oracle.first_hits(desc, cam, params(LAW_W, LAW_H, spp, seed=seed, integrator=ffi.VK_INTEGRATOR_SCATTER), 0, spp)
        return fh["origin"], fh["time"]

    def by_emulator(seed, spp):
        rays, _ = emu_film_ffi.emit(cam, params(LAW_W, LAW_H, spp, seed=seed, integrator=ffi.VK_INTEGRATOR_SCATTER), 0, 0, LAW_W, LAW_H, 0, spp)
        o, _, t = in_id_order(rays, (LAW_H, LAW_W, spp))
        return o, t
    for who, route in (("oracle", by_oracle), ("emulator", by_emulator)):
        stats, ctl, failing = hold_laws(route, oracle, c, f"{who} {name}")
        worst = max(stats, key=lambda k: abs(stats[k]["z"]))
        print(f"\n   {who} {name}: {len(stats)} statistics of {LAW_W * LAW_H * LAW_SPP} samples, worst |z| {abs(stats[worst]['z']):.2f} ({worst}), "
              f"repeated {failing}; E r^2 {stats['E r^2']['got']:.5f} +- {stats['E r^2']['se']:.5f}, E time {stats['E time']['got']:.5f} +- "
              f"{stats['E time']['se']:.5f}; controls z " + ", ".join(f"{k} {z:.1f}" for k, z in ctl.items()))


# ================================================================ 3. frames: a defocused edge
EDGE_FOCUS, EDGE_APERTURE, EDGE_SPP, EDGE_SEED = 4.0, 2.0, 512, 31
EDGE_CASES = {           # name -> (axis the profile runs along, depth of the emitter, where its edge is)
    "vertical-D2": (0, 2.0, 0.07), "vertical-D8": (0, 8.0, 0.3), "horizontal-D2": (1, 2.0, 0.07), "horizontal-D8": (1, 8.0, 0.3)}
EDGE_C = dict(lookfrom=(0, 0, 0), lookat=(0, 0, -1), vup=(0, 1, 0), vfov=40.0, aspect=1.0, aperture=EDGE_APERTURE, focus=EDGE_FOCUS, t0=0.0, t1=1.0)


def edge_case(name):
    """(owner, desc, cam, f64 cam, p, axis): a DiffuseLight xy_rect covering x >= edge (axis 0, on a 33 x 16 frame whose 16 rows are
    replicas) or y >= edge (axis 1, 16 x 33), far beyond the frame the other way, at z = -depth; black background, max_depth 1"""
    axis, depth, edge = EDGE_CASES[name]
    d = Desc()
    far = max(3.0, depth)          # beyond every ray of the frame (|x|, |y| < 0.5 depth + 0.5); geometry_ref's edge margin is relative to the rect's size
    r = d.xy_rect(edge, far, -far, far, -depth, d.light(*LE)) if axis == 0 else d.xy_rect(-far, far, edge, far, -depth, d.light(*LE))
    desc = d.finish(d.big_box(r, d.sphere((0, 0, 500), 0.1, d.lambertian(0, 0, 0))))
    cam, c64 = camera_pair(EDGE_C)
    w, h = (33, 16) if axis == 0 else (16, 33)
    p = params(w, h, EDGE_SPP, max_depth=1, seed=EDGE_SEED, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SOLID)
    return d, desc, cam, c64, p, axis


def counts_of(img, spp, what):
    """a frame of Le = (1, 0.5, 2) emitters under a black background at max_depth 1, as per-pixel counts (exact: spp is a power of two)"""
    k = img[..., 0].astype(f64) * spp
    assert (k == np.round(k)).all() and (img[..., 1] * 2 == img[..., 0]).all() and (img[..., 2] == img[..., 0] * 2).all(), what
    return k.astype(np.int64)


def edge_law(name):
    axis, depth, edge = EDGE_CASES[name]
    _, c64 = camera_pair(EDGE_C)
    return L.edge_coverage(c64, EDGE_FOCUS, depth, edge, axis, 33)


def hold_edge(name, counts, what):
    """per-pixel counts (height, width) against the law: the conditions, every partial column within 4 SE, the pooled chi-square within
    its 4-sigma range.  Returns (chi2, m, z, worst |z|)."""
    axis, depth, edge = EDGE_CASES[name]
    p, exact = edge_law(name)
    k = counts.sum(0) if axis == 0 else counts.sum(1)
    n = 16 * EDGE_SPP
    partial = exact < 0
    assert partial.sum() >= 8, f"{what}: only {partial.sum()} partial columns"
    assert (k[exact == 0] == 0).all() and (k[exact == 1] == n).all(), f"{what}: a column the law puts at 0 or 1 is not"
    assert (exact == 0).any() and (exact == 1).any()
    dev = np.abs(k / n - p)[partial]
    assert (dev <= 4.0 * np.sqrt(p * (1 - p) / n)[partial]).all(), f"{what}: columns {k[partial]} of {n}, the law {p[partial]}"
    chi2, m, z, worst = L.pooled(k, n, p, partial)
    assert abs(z) <= 4.0, f"{what}: pooled chi-square {chi2:.1f} over {m} columns: z = {z:.2f}"
    return chi2, m, z, worst


def edge_controls(name, counts):
    """the pooled z of the two misread profiles on the same counts"""
    axis, depth, edge = EDGE_CASES[name]
    _, c64 = camera_pair(EDGE_C)
    _, exact = edge_law(name)
    k = counts.sum(0) if axis == 0 else counts.sum(1)
    out = {}
    for ctl, kw in (("uniform in radius", dict(share=L.radius_uniform_share, m=512)), ("R = aperture", dict(radius=EDGE_APERTURE))):
        p, _ = L.edge_coverage(c64, EDGE_FOCUS, depth, edge, axis, 33, **kw)
        sel = (exact < 0) & (p > 0) & (p < 1)
        out[ctl] = L.pooled(k, 16 * EDGE_SPP, p, sel)[2]
    return out


_sim = {}


def simulated(oracle, key, c64, desc, seed, width, height, spp):
    if key not in _sim:
        _sim[key] = L.simulate_counts(oracle.draws, c64, G.Scene(desc), seed, width, height, spp)
    return _sim[key]


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_defocused_edge(name, oracle, emu):
    d, desc, cam, c64, p, axis = edge_case(name)
    # the reference side alone first: the f64 simulation of get_ray meets the law and rejects both controls
    sim, unstable = simulated(oracle, name, c64, desc, EDGE_SEED, p.width, p.height, EDGE_SPP)
    assert unstable <= L.MAX_EXCLUDED
    chi2, m, z, worst = hold_edge(name, sim, f"f64 {name}")
    ctl = edge_controls(name, sim)
    print(f"\n   {name}: f64 simulation: {m} partial columns, chi2 {chi2:.1f}, z {z:.2f}, worst column |z| {worst:.2f}; controls z "
          + ", ".join(f"{k} {v:.1f}" for k, v in ctl.items()))
    for k, v in ctl.items():
        assert v > 8.0, f"{name}: the control '{k}' is not rejected by the f64 simulation at {EDGE_SPP} samples: z = {v:.2f}"
    img_o, _ = oracle.render(desc, cam, p)
    img_e = emu.render_samples(desc, cam, p)[0]
    k_o, k_e = counts_of(img_o, EDGE_SPP, "oracle"), counts_of(img_e, EDGE_SPP, "emulator")
    assert np.array_equal(k_o, k_e), name
    chi2, m, z, worst = hold_edge(name, k_o, f"oracle {name}")
    for kk, v in edge_controls(name, k_o).items():
        assert v > 8.0, (name, kk, v)
    print(f"   {name}: oracle = emulator: chi2 {chi2:.1f}, z {z:.2f}, worst column |z| {worst:.2f}; {int(np.abs(k_o - sim).sum())} samples "
          f"differ from the f64 simulation's")


# ================================================================ 3. frames: the stratified quadrature, and a sphere through the lens
QUAD_MJ, QUAD_ML = 4, 64


def quadrature_pixels(c64, sc, width, height, pixels, mj, ml, mt=1, chunk=1 << 20):
    """the coverage of the given pixels [(x, y)] by emitters' front faces: midpoints of mj x mj strata of the jitter, of
    camera_laws_ref.lens_grid(ml)'s strata of the lens and of mt strata of the shutter, each an f64 ray of get_ray's form
    (main.rs:111-120) against geometry_ref.closest_hit"""
    j = (np.arange(mj) + 0.5) / mj
    grid = L.lens_grid(ml)
    tt = c64["time0"] + (np.arange(mt) + 0.5) / mt * (c64["time1"] - c64["time0"])
    jx, jy, li, tm = (a.reshape(-1) for a in np.meshgrid(j, j, np.arange(len(grid)), tt, indexing="ij"))
    rd = grid[li] * c64["lens_radius"]
    o = c64["origin"] + rd[:, 0:1] * c64["u"] + rd[:, 1:2] * c64["v"]
    per = max(1, chunk // len(jx))
    out = []
    for i in range(0, len(pixels), per):
        xy = np.array(pixels[i:i + per], f64)
        s, t = (xy[:, 0:1] + jx) / (width - 1), (xy[:, 1:2] + jy) / (height - 1)
        oo = np.broadcast_to(o, s.shape + (3,))
        hit, _ = G.closest_hit(sc, oo.reshape(-1, 3), (G.focus_point(c64, s, t) - oo).reshape(-1, 3), np.broadcast_to(tm, s.shape).reshape(-1))
        out.append(L.lit(sc, hit).reshape(s.shape).mean(1))
    return np.concatenate(out)


def test_the_quadrature_meets_the_segment_formula():
    """on the edge cases' middle row (column), at the resolution the sphere's law is computed with: the stratified quadrature against
    edge_coverage within a tenth of the smallest SE the sphere's frame compares it with"""
    law_s, _ = sphere_law()
    tol = 0.1 * np.sqrt(law_s * (1 - law_s) / SPH_SPP)[sphere_compared(law_s)].min()
    for name in ("vertical-D2", "horizontal-D8"):
        d, desc, cam, c64, p, axis = edge_case(name)
        law, exact = edge_law(name)
        cols = np.flatnonzero(exact < 0)
        cols = np.arange(cols[0] - 1, cols[-1] + 2)                 # the partial ones and one beyond each end
        pixels = [(i, 7) if axis == 0 else (7, i) for i in cols]
        q = quadrature_pixels(c64, G.Scene(desc), p.width, p.height, pixels, QUAD_MJ, QUAD_ML)
        print(f"\n   {name}: quadrature - formula {np.abs(q - law[cols]).max():.3g} over {len(cols)} columns; a tenth of the sphere frame's smallest SE {tol:.3g}")
        assert np.abs(q - law[cols]).max() <= tol
        assert (q[exact[cols] == 0] == 0).all() and (q[exact[cols] == 1] == 1).all()


# The law of a pixel is a 4-D integral of an indicator: a midpoint rule of N points errs by about N^-5/8, so 1e-3 costs 1e5 rays a pixel
# and 1e-4 would cost 4e6.  The frame is therefore sized for the quadrature: 16 x 12 pixels (small against the blur, so that 4 x 4 jitter
# points do) at 128 samples, the law on every second pixel of every second row (48), a pixel compared where 0.05 <= p <= 0.95 (SE >=
# 0.019, a tenth of it 1.9e-3), and the quadrature held to itself at twice the resolution on every eighth of those pixels.
SPH_W, SPH_H, SPH_SPP, SPH_SEED = 16, 12, 128, 41
SPH_PIXELS = [(x, y) for y in range(1, SPH_H, 2) for x in range(y // 2 % 2, SPH_W, 2)]
SPH_C = dict(EDGE_C, aspect=SPH_W / SPH_H)
_sphere_law = {}


def sphere_case():
    """an emissive sphere of radius 0.5 at depth 2 among four black Lambertian ones, two of which hide parts of it, through the edge's
    lens: spheres only, small enough for the sphere-only kernel instance with the scene in LDS"""
    d = Desc()
    black = d.lambertian(0, 0, 0)
    refs = [d.sphere((0.1, -0.05, -2.0), 0.5, d.light(*LE)), d.sphere((-0.45, 0.2, -1.3), 0.15, black), d.sphere((0.5, -0.3, -1.5), 0.2, black),
            d.sphere((0.0, 0.6, -3.0), 0.4, black), d.sphere((-0.8, -0.5, -4.0), 0.6, black)]
    objs = []
    for ref, s in zip(refs, d.spheres):
        c = np.array(list(s.center), f32)
        objs.append((ref, c - f32(s.radius), c + f32(s.radius)))
    desc = d.finish(T._tree_of_spheres(d, objs)[0], [])
    cam, c64 = camera_pair(SPH_C)
    p = params(SPH_W, SPH_H, SPH_SPP, max_depth=1, seed=SPH_SEED, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SOLID)
    return d, desc, cam, c64, p


def sphere_compared(law):
    return (law >= 0.05) & (law <= 0.95)


def sphere_law(check=False):
    """(p of SPH_PIXELS, the quadrature's error against itself at twice the resolution — of the jitter, then of the lens, the two
    summed — on every eighth of them; None unless asked for)"""
    d, desc, cam, c64, p = sphere_case()
    sc = G.Scene(desc)
    if "p" not in _sphere_law:
        _sphere_law["p"] = quadrature_pixels(c64, sc, SPH_W, SPH_H, SPH_PIXELS, QUAD_MJ, QUAD_ML)
    if check and "err" not in _sphere_law:
        sub = SPH_PIXELS[::8]
        qj = quadrature_pixels(c64, sc, SPH_W, SPH_H, sub, 2 * QUAD_MJ, QUAD_ML)
        ql = quadrature_pixels(c64, sc, SPH_W, SPH_H, sub, QUAD_MJ, 2 * QUAD_ML)
        _sphere_law["err"] = float((np.abs(qj - _sphere_law["p"][::8]) + np.abs(ql - _sphere_law["p"][::8])).max())
    return _sphere_law["p"], _sphere_law.get("err")


def hold_cells(counts, p, n, what, z_max, min_partial, compared=None):
    """counts against coverages, cell by cell: (chi2, m, z, worst |z|) over the compared cells (default: the partial ones), each within
    z_max and the pooled chi-square within 4 sigma; cells the law puts at exactly 0 or 1 are exactly that"""
    partial = (p > 0) & (p < 1) if compared is None else compared
    assert partial.sum() >= min_partial, f"{what}: only {partial.sum()} partial pixels"
    assert (counts[p == 0] == 0).all() and (counts[p == 1] == n).all(), what
    chi2, m, z, worst = L.pooled(counts, n, p, partial)
    assert worst <= z_max, f"{what}: a pixel at |z| = {worst:.2f}"
    assert abs(z) <= 4.0, f"{what}: pooled chi-square {chi2:.1f} over {m} pixels: z = {z:.2f}"
    return chi2, m, z, worst


def sphere_counts(counts):
    """a frame's counts (height, width) at SPH_PIXELS"""
    return np.array([counts[y, x] for x, y in SPH_PIXELS])


def hold_sphere(counts, what):
    law, _ = sphere_law()
    return hold_cells(sphere_counts(counts), law, SPH_SPP, what, 4.0, 30, sphere_compared(law))


def test_defocused_sphere(oracle, emu):
    d, desc, cam, c64, p = sphere_case()
    law, err = sphere_law(check=True)
    se = np.sqrt(law * (1 - law) / SPH_SPP)[sphere_compared(law)].min()
    assert err <= 0.1 * se, (err, se)
    sim, unstable = simulated(oracle, "sphere", c64, desc, SPH_SEED, SPH_W, SPH_H, SPH_SPP)
    assert unstable <= L.MAX_EXCLUDED
    hold_sphere(sim, "f64 sphere")
    k_o, k_e = counts_of(oracle.render(desc, cam, p)[0], SPH_SPP, "oracle"), counts_of(emu.render_samples(desc, cam, p)[0], SPH_SPP, "emulator")
    assert np.array_equal(k_o, k_e)
    chi2, m, z, worst = hold_sphere(k_o, "oracle sphere")
    print(f"\n   sphere: quadrature error {err:.3g}, smallest SE {se:.3g}; oracle = emulator: {m} pixels compared, "
          f"chi2 {chi2:.1f}, z {z:.2f}, worst pixel |z| {worst:.2f}; {int(np.abs(k_o - sim).sum())} samples differ from the f64 simulation's")


# ================================================================ 3. frames: sphere clouds under a lens
CLOUD_APERTURE = 0.6
_cloud_cache = {}


def lens_cloud(name):
    """test_geometry.cloud with its camera's aperture opened to 0.6 (the camera's other fields are Camera::new's for any aperture,
    main.rs:71-109)"""
    d, desc, cam, p, scale = T.cloud(name)
    cam = ffi.Camera.from_buffer_copy(cam)
    cam.lens_radius = CLOUD_APERTURE / 2.0
    return d, desc, cam, p, scale


def lens_cloud_winners(name, oracle):
    """per sample [pixel * spp + s]: the sphere the f64 closest hit of part 1's f64 ray names (-1: none), whether the ray is stable, the
    face"""
    if name not in _cloud_cache:
        d, desc, cam, p, scale = lens_cloud(name)
        c64 = {k: np.array(list(getattr(cam, k)), f64) for k in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w")}
        c64.update(lens_radius=float(cam.lens_radius), time0=float(cam.time0), time1=float(cam.time1))
        st = streams(oracle, T.CLOUD_SEED, T.CLOUD_W, T.CLOUD_H, 0, T.CLOUD_SPP)
        o, dd, t, bad = L.get_ray(c64, st)
        hit, record = G.closest_hit(G.Scene(desc), o.reshape(-1, 3), dd.reshape(-1, 3), t.reshape(-1))
        winner = np.where(hit["hit"], (hit["object"] & G.INDEX_MASK).astype(np.int64), -1)
        _cloud_cache[name] = (winner, G.stable(record) & ~bad.reshape(-1), hit["front"])
    return _cloud_cache[name]


def check_lens_cloud(name, samples, oracle, what):
    """test_geometry.check_cloud's rules with the lens: every sample that names a sphere names the f64 winner of its own f64 ray, B only
    where that ray misses, black on an emitter exactly on its back face; at most 1 % unstable; half of the samples name a sphere"""
    d, desc, cam, p, scale = lens_cloud(name)
    winner, ok, front = lens_cloud_winners(name, oracle)
    assert 1.0 - ok.mean() <= G.MAX_EXCLUDED, f"{what}: {1 - ok.mean():.4f} unstable"
    k = T.cloud_decode(samples, scale)
    named = k >= 0
    bad = np.flatnonzero(ok & named & (k != winner))
    assert len(bad) == 0, f"{what}: {len(bad)} samples name another sphere than the f64 winner; first {bad[0]}: {k[bad[0]]} for {winner[bad[0]]}"
    bad = np.flatnonzero(ok & ((k == -1) != (winner == -1)))
    assert len(bad) == 0, f"{what}: {len(bad)} samples disagree on the miss; first {bad[0]}: {k[bad[0]]} for {winner[bad[0]]}"
    if scale == 1.0:
        bad = np.flatnonzero(ok & (winner >= 0) & ((k == -2) != ~front))
        assert len(bad) == 0, f"{what}: {len(bad)} samples disagree on the face; first {bad[0]}"
    assert named.mean() >= 0.5, f"{what}: only {named.mean():.3f} of the samples name a sphere"
    return float(named.mean()), float(1.0 - ok.mean())


@pytest.mark.parametrize("name", T.CLOUDS)
def test_cloud_under_a_lens(name, oracle, emu):
    d, desc, cam, p, scale = lens_cloud(name)
    share, excluded = check_lens_cloud(name, oracle.render_samples(desc, cam, p)[1], oracle, f"oracle {name}")
    # the lens moves the winners: a pass must not be the pinhole's
    pin = T.cloud_winners(name, oracle)[0]
    moved = float((pin != lens_cloud_winners(name, oracle)[0]).mean())
    print(f"\n   {name} under aperture {CLOUD_APERTURE}: {share:.3f} of the samples name a sphere, {excluded:.4%} unstable, {moved:.3f} of the winners "
          f"differ from the pinhole's")
    assert moved > 0.02
    for flags in (0, ffi.VK_SCENE_REFERENCE_TREE, ffi.VK_SCENE_FAST_ACCEL):
        desc.contents.flags = flags
        check_lens_cloud(name, emu.render_samples(desc, cam, p)[1], oracle, f"emulator {name} flags {flags}")


# ================================================================ 3. frames: motion blur
MB_W, MB_H, MB_SPP, MB_SEED = 24, 12, 2048, 51
MB_C = dict(lookfrom=(0, 0, 0), lookat=(0, 0, -1), vup=(0, 1, 0), vfov=40.0, aspect=2.0, aperture=0.0, focus=10.0, t0=0.25, t1=1.75)
MB_SPHERE = dict(c0=(-0.75, 0.3, -10.0), c1=(0.7, 0.5, -10.0), s0=0.6, s1=1.2, radius=2.0)     # its shutter is (0.6, 1.2): f32 values below
MB_LENS_C = dict(MB_C, aperture=2.0, focus=5.0)                                                # the same sphere, focused at half its distance
MB_LENS_W, MB_LENS_H, MB_LENS_SPP = 24, 12, 512


def moving_case(c=MB_C, width=MB_W, height=MB_H, spp=MB_SPP):
    d = Desc()
    m = MB_SPHERE
    s = d.moving_sphere(m["c0"], m["c1"], m["s0"], m["s1"], m["radius"], d.light(*LE))
    desc = d.finish(d.big_box(s, d.sphere((0, 0, 500), 0.1, d.lambertian(0, 0, 0))))
    cam, c64 = camera_pair(c)
    p = params(width, height, spp, max_depth=1, seed=MB_SEED, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SOLID)
    return d, desc, cam, c64, p


_mb_law = {}


def moving_law(**control):
    """the pinhole's per-pixel coverage (moving_coverage) with the sphere's f32 shutter; cached"""
    key = tuple(sorted(control.items()))
    if key not in _mb_law:
        _, c64 = camera_pair(MB_C)
        m = MB_SPHERE
        _mb_law[key] = L.moving_coverage(c64, MB_W, MB_H, m["c0"], m["c1"], float(f32(m["s0"])), float(f32(m["s1"])), m["radius"], **control)
    return _mb_law[key]


MB_CONTROLS = {"centre clamped": dict(clamp=True), "camera shutter [0, 1)": dict(shutter=(0.0, 1.0)), "interpolated over the camera's shutter": dict(over_camera=True)}


def moving_controls(counts):
    law = moving_law()
    partial = (law > 0) & (law < 1)
    out = {}
    for name, kw in MB_CONTROLS.items():
        p = moving_law(**kw)
        # a control that puts a pixel at exactly 0 or 1 where samples say otherwise is refuted outright there; the statistic is pooled
        # over the pixels where both profiles are partial
        sel = partial & (p > 0) & (p < 1)
        out[name] = L.pooled(counts, MB_SPP, p, sel)[2]
    return out


def test_motion_blur(oracle, emu):
    d, desc, cam, c64, p = moving_case()
    m = MB_SPHERE
    law = moving_law()
    fine = L.moving_coverage(c64, MB_W, MB_H, m["c0"], m["c1"], float(f32(m["s0"])), float(f32(m["s1"])), m["radius"], m=48)
    partial = (law > 0) & (law < 1)
    se = np.sqrt(law * (1 - law) / MB_SPP)
    err = np.abs(law - fine)
    assert (err[partial] <= 0.1 * se[partial]).all() and (err[~partial] == 0).all(), (err[partial] / se[partial]).max()
    # the centre crosses about six pixels during the camera's shutter, and is seen outside its own
    px = (MB_W - 1) / (2.0 * math.tan(math.radians(20.0)) * 2.0 * 10.0)
    speed = (m["c1"][0] - m["c0"][0]) / (m["s1"] - m["s0"])
    assert 5.0 < speed * 1.5 * px < 7.0
    sim, unstable = simulated(oracle, "moving", c64, desc, MB_SEED, MB_W, MB_H, MB_SPP)
    assert unstable <= L.MAX_EXCLUDED
    chi2, mm, z, worst = hold_cells(sim, law, MB_SPP, "f64 motion blur", 5.0, 60)
    ctl = moving_controls(sim)
    print(f"\n   motion blur: quadrature error / SE {(err[partial] / se[partial]).max():.3g}; f64 simulation: {mm} partial pixels, chi2 {chi2:.1f}, "
          f"z {z:.2f}, worst pixel |z| {worst:.2f}; controls z " + ", ".join(f"{k} {v:.1f}" for k, v in ctl.items()))
    for k, v in ctl.items():
        assert v > 8.0, f"the control '{k}' is not rejected by the f64 simulation: z = {v:.2f}"
    k_o, k_e = counts_of(oracle.render(desc, cam, p)[0], MB_SPP, "oracle"), counts_of(emu.render_samples(desc, cam, p)[0], MB_SPP, "emulator")
    assert np.array_equal(k_o, k_e)
    chi2, mm, z, worst = hold_cells(k_o, law, MB_SPP, "oracle motion blur", 5.0, 60)
    for k, v in moving_controls(k_o).items():
        assert v > 8.0, (k, v)
    print(f"   motion blur: oracle = emulator: chi2 {chi2:.1f}, z {z:.2f}, worst pixel |z| {worst:.2f}; {int(np.abs(k_o - sim).sum())} samples differ "
          f"from the f64 simulation's")


MBL_MJ, MBL_ML, MBL_ROWS = 6, 32, (3, 7)
_mbl_law = {}


def moving_lens_law(check=False):
    """the moving sphere through the R = 1 lens focused at half its distance: the quadrature over jitter and lens of the exact share
    of the shutter (camera_laws_ref.moving_coverage), and — where asked for — its error against itself at twice the resolution of
    the jitter, then of the lens, the two summed, on two rows through the sphere"""
    _, c64 = camera_pair(MB_LENS_C)
    m = MB_SPHERE
    args = (c64, MB_LENS_W, MB_LENS_H, m["c0"], m["c1"], float(f32(m["s0"])), float(f32(m["s1"])), m["radius"])
    if "p" not in _mbl_law:
        _mbl_law["p"] = L.moving_coverage(*args, m=MBL_MJ, ml=MBL_ML)
    if check and "err" not in _mbl_law:
        rows = list(MBL_ROWS)
        qj, ql = L.moving_coverage(*args, m=2 * MBL_MJ, ml=MBL_ML, rows=rows), L.moving_coverage(*args, m=MBL_MJ, ml=2 * MBL_ML, rows=rows)
        _mbl_law["err"] = float((np.abs(qj - _mbl_law["p"]) + np.abs(ql - _mbl_law["p"]))[rows].max())
    return _mbl_law["p"], _mbl_law.get("err")


def hold_moving_lens(counts, what):
    """a pixel is compared where 0.05 <= p <= 0.95 (the quadrature is held to a tenth of the smallest SE among those)"""
    law, _ = moving_lens_law()
    return hold_cells(counts, law, MB_LENS_SPP, what, 5.0, 30, (law >= 0.05) & (law <= 0.95))


def test_motion_blur_through_a_lens(oracle, emu):
    d, desc, cam, c64, p = moving_case(MB_LENS_C, MB_LENS_W, MB_LENS_H, MB_LENS_SPP)
    law, err = moving_lens_law(check=True)
    compared = (law >= 0.05) & (law <= 0.95)
    se = np.sqrt(law * (1 - law) / MB_LENS_SPP)[compared].min()
    assert err <= 0.1 * se, (err, se)
    # the 5-D midpoint quadrature against closest_hit, time included, agrees on the middle row as far as an indicator's quadrature can
    row = [(x, 7) for x in range(4, 20)]
    q5 = quadrature_pixels(c64, G.Scene(desc), MB_LENS_W, MB_LENS_H, row, 2, 24, 24)
    assert np.abs(q5 - law[7, 4:20]).max() <= 0.02, np.abs(q5 - law[7, 4:20]).max()
    k_o, k_e = counts_of(oracle.render(desc, cam, p)[0], MB_LENS_SPP, "oracle"), counts_of(emu.render_samples(desc, cam, p)[0], MB_LENS_SPP, "emulator")
    assert np.array_equal(k_o, k_e)
    chi2, mm, z, worst = hold_moving_lens(k_o, "oracle motion blur through a lens")
    print(f"\n   motion blur through a lens: quadrature error {err:.3g}, smallest SE {se:.3g}, 5-D midpoints - law {np.abs(q5 - law[7, 4:20]).max():.3g}; "
          f"oracle = emulator: {mm} pixels compared, chi2 {chi2:.1f}, z {z:.2f}, worst pixel |z| {worst:.2f}")
