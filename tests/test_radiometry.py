"""The integrators against closed-form radiometry, on the CPU: the oracle (oracle/oracle.cpp) and the emulator (vk_trace.h on the host).

Every other shading test compares one restatement of the reference with another; both were written from the same reading of
material.rs, hittable.rs and main.rs, and a shared misreading — a light pdf without its cosine, a depth test off by one, a mixture weight
applied twice — passes them bit for bit.  Here the expected values are f64 closed forms (tests/radiometry_ref.py) that come from the
reference's lines alone: five tiny scenes, the statistical rule of that module's docstring, and a power control per family that the
same samples must reject.

Routes.  The emulator answers rays, points and frames per sample (emu_queries_ffi, emu_ffi).  The oracle renders frames only: a ray is
put to it through a camera of 1e-6 degrees whose 2 x 2 pixels all look along that ray (to f32 rounding), and the cases that need points
(vk_trace_irradiance) have no oracle route — the frame of the same scene stands in for them.  The emulator's samples are also folded
into replica means and held to the rule as tests/test_gpu_radiometry.py holds the public calls, which return the same bytes.

Two properties of the reference that no closed form pins are asserted as they are (radiometry_ref.property_a / property_b):
a sphere in `lights` biases the PDF integrator, and a FlipFace'd entry in `lights` turns half of the samples into NaN."""
import math

import numpy as np
import pytest

import radiometry_ref as R

NAMES = list(R.STATISTICAL)
ORACLE_NAMES = [n for n in NAMES if not n.startswith(("sphere-irradiance", "rect-tilted"))]


@pytest.fixture(scope="module")
def queries(built):
    import emu_queries_ffi
    emu_queries_ffi.load()
    return emu_queries_ffi


def emu_samples(case, queries, emu):
    owner, desc = case.scene()
    kw = dict(case.kw, samples_per_ray=case.spp)
    if case.route == "rays":
        return queries.radiance_samples(desc, case.items, **kw)[0]
    if case.route == "points":
        return queries.irradiance_samples(desc, case.items, **kw)[0]
    return emu.render_samples(desc, case.cam, case.render_params())[1]


def ray_camera(o, d):
    """a camera at o whose every ray is d to f32 rounding: 1e-6 degrees wide, looking along d"""
    o, d = np.asarray(o, float), np.asarray(d, float)
    vup = (0, 0, 1) if abs(d[1]) >= max(abs(d[0]), abs(d[2])) else (0, 1, 0)
    return R.camera(tuple(o), tuple(o + d), vfov=1e-6, aspect=1.0, aperture=0.0, focus=float(np.linalg.norm(d)), vup=vup)


def oracle_samples(case, oracle):
    """the case's samples from oracle.render_samples: a frame as it is; the copies of a ray as the 2 x 2 pixels of ray_camera"""
    owner, desc = case.scene()
    if case.route == "frame":
        return oracle.render_samples(desc, case.cam, case.render_params())[1]
    out = np.zeros((len(case.items), case.spp, 4), np.float32)
    for g in range(len(case.want)):
        mine = np.flatnonzero(case.group == g)
        n = len(mine) * case.spp
        assert n % 4 == 0
        p = R.params(2, 2, n // 4, max_depth=case.kw["max_depth"], seed=case.kw["seed"] + g, integrator=case.kw["integrator"],
                     background=case.kw["background"], bg=case.kw["background_color"])
        item = case.items[mine[0]]
        out[mine] = oracle.render_samples(desc, ray_camera(item["origin"], item["direction"]), p)[1].reshape(len(mine), case.spp, 4)
    return out


def replica_means(case, samples):
    """what the public call returns for the same submission: per record (per pixel) the mean of its samples, a non-finite one as 0"""
    x = np.asarray(samples, np.float64)[..., :3]
    if case.route == "frame":
        w, h = case.size
        x = x.reshape(h * w, case.spp, 3)
    x = np.where(np.isfinite(x).all(-1, keepdims=True), x, 0.0)
    return x.mean(1)


def report(name, route, results):
    for g, (mean, se, z) in enumerate(results):
        print(f"\n   {name}[{g}] {route}: mean {np.round(mean, 6)} se {np.round(se, 6)} z {np.round(z, 2)}", end="")


# ---------------------------------------------------------------- the reference's own checks
def test_form_factors_against_quadrature_and_each_other():
    """both formulas against a midpoint rule of h^2 / (pi r^4) on a 4000 x 4000 grid — whose own error, (cell^2 / 24) |laplace f| / f
    with cells of 2.5e-4 x 3.75e-4, is a few 1e-8 — and against each other for the normal (0, 1, 0)"""
    for (x, z) in R.RECT_XZ:
        F = R.rect_form_factor_parallel(x, z, R.RECT, R.RECT_H)
        P = R.polygon_form_factor((x, 0.0, z), (0, 1, 0), R.RECT_VERTS)
        assert abs(P / F - 1.0) < 1e-12, (x, z, F, P)
    x, z = R.RECT_XZ[1]
    F = R.rect_form_factor_parallel(x, z, R.RECT, R.RECT_H)
    Q = R.quadrature_parallel(x, z, R.RECT, R.RECT_H, m=4000)
    print(f"\n   F({x}, {z}) = {F:.12f}, quadrature {Q:.12f}, relative {abs(Q / F - 1):.2e}")
    assert abs(Q / F - 1.0) < 1e-7
    # the odd corner term: a rectangle that straddles the element equals the sum of its four quadrants
    assert abs(R.rect_form_factor_parallel(0, 0, (-1, 2, -3, 4), 1.5) - sum(R._corner(a, b, 1.5) for a in (1, 2) for b in (3, 4))) < 1e-15
    # a tilted receiver: Lambert's formula against a quadrature of cos cos' / (pi r^2) over the polygon
    p, n = (np.asarray(v, float) for v in R.TILTED[0])
    n = n / np.linalg.norm(n)
    m = 2000
    xs = R.RECT[0] + (np.arange(m) + 0.5) * (R.RECT[1] - R.RECT[0]) / m
    zs = R.RECT[2] + (np.arange(m) + 0.5) * (R.RECT[3] - R.RECT[2]) / m
    r = np.stack(np.broadcast_arrays(xs[:, None] - p[0], R.RECT_H - p[1], zs[None, :] - p[2]), -1)
    r2 = (r * r).sum(-1)
    q = ((r @ n) * r[..., 1] / (math.pi * r2 * r2)).sum() * (R.RECT[1] - R.RECT[0]) * (R.RECT[3] - R.RECT[2]) / m ** 2
    assert abs(q / R.polygon_form_factor(p, n, R.RECT_VERTS) - 1.0) < 1e-6
    with pytest.raises(AssertionError):
        R.polygon_form_factor((0, 0, 0), (1, 0, 0), R.RECT_VERTS)          # the polygon crosses that horizon


def test_series_and_chain():
    a, Le = np.asarray(R.SPHERE_A), np.asarray(R.SPHERE_LE)
    q = a * (1 - R.SPHERE_F)
    terms = [Le * R.SPHERE_F * q ** k for k in range(50)]
    for D in R.SPHERE_DEPTHS:
        np.testing.assert_allclose(R.integrating_sphere(a, R.SPHERE_F, Le, D), sum(terms[:D]), rtol=1e-14)
    assert abs(R.GLASS_R0 - 0.04) < 1e-15
    assert R.glass_diameter_chain(0.04, 1) == (0.0, 0.0) and R.glass_diameter_chain(0.04, 2) == (0.04, 0.0)
    np.testing.assert_allclose(R.glass_diameter_chain(0.04, 3), (0.04, 0.96 ** 2), rtol=1e-15)
    np.testing.assert_allclose(R.glass_diameter_chain(0.04, 4), (0.04 + 0.96 ** 2 * 0.04, 0.96 ** 2), rtol=1e-15)
    back, fwd = R.glass_diameter_chain(0.04, 50)
    assert abs(fwd - 0.96 / 1.04) < 1e-15 and abs(back + fwd - 1.0) < 1e-15
    # the same chain as powers of its transition matrix over (in going up, in going down, out back, out forward)
    T = np.zeros((4, 4))
    T[0] = [0, 0.04, 0, 0.96]
    T[1] = [0.04, 0, 0.96, 0]
    T[2, 2] = T[3, 3] = 1
    for D in R.GLASS_DEPTHS[1:]:
        v = np.array([0.96, 0, 0.04, 0]) @ np.linalg.matrix_power(T, D - 2)     # after segment 2: inside (0.96) or gone back (0.04)
        np.testing.assert_allclose(R.glass_diameter_chain(0.04, D), (v[2], v[3]), rtol=1e-13, atol=1e-18)


def test_pixel_centres_stand_for_their_footprints():
    err = R.footprint_error()
    print(f"\n   largest |mean F over a pixel's footprint / F at its centre - 1| = {err:.2e}")
    assert err < 1e-4


def test_z_scores_keep_dropped_samples_in_n():
    x = np.ones((8, 3))
    x[0] = np.nan
    x[1, 2] = np.inf
    mean, se, _ = R.z_scores(x, 0.75)
    np.testing.assert_allclose(mean, 0.75)
    np.testing.assert_allclose(se, np.std([0, 0, 1, 1, 1, 1, 1, 1], ddof=1) / math.sqrt(8))
    with pytest.raises(AssertionError, match="vacuous"):
        R.check(np.random.default_rng(0).normal(1, 1, (100, 3)), 1.0, "wide")


# ---------------------------------------------------------------- the closed forms
@pytest.mark.parametrize("name", NAMES)
def test_emulator_meets_the_closed_form(name, queries, emu):
    case = R.STATISTICAL[name]()
    samples = emu_samples(case, queries, emu)
    report(name, "samples", case.check_samples(samples, "emulator"))
    report(name, "replica means", case.check_means(replica_means(case, samples), "emulator, replica means"))


@pytest.mark.parametrize("name", ORACLE_NAMES)
def test_oracle_meets_the_closed_form(name, oracle):
    case = R.STATISTICAL[name]()
    report(name, "samples", case.check_samples(oracle_samples(case, oracle), "oracle"))


@pytest.mark.parametrize("integrator", [R.PDF, R.SCATTER], ids=["pdf", "scatter"])
def test_mirror_is_exact(integrator, queries, emu, oracle):
    case = R.mirror(integrator)
    dev_e = R.mirror_deviation(emu_samples(case, queries, emu))
    dev_o = R.mirror_deviation(oracle_samples(case, oracle))
    print(f"\n   largest relative deviation from f64: emulator {dev_e:.2e}, oracle {dev_o:.2e}")
    assert dev_e <= R.MIRROR_TOL and dev_o <= R.MIRROR_TOL


# ---------------------------------------------------------------- what the closed forms cannot pin
def test_a_sphere_in_lights_biases_the_pdf_integrator(queries, emu):
    """property A: NOT the radiometric value — blue differs from it by |z| > 4 at depth 50, upwards — so that nobody corrects
    random_to_sphere away from the reference unnoticed.  (Measured on the emulator: +1.0 % / +1.7 % / +2.7 %, z 2.7 / 7.2 / 8.3.)"""
    case = R.property_a()
    samples = emu_samples(case, queries, emu)
    mean, se, z = R.z_scores(samples[..., :3], case.want[0])
    print(f"\n   mean / radiometric - 1 = {np.round(mean / case.want[0] - 1, 4)}, z {np.round(z, 2)}")
    assert (se <= R.SE_CAP * case.want[0]).all()
    assert z[2] > R.Z_MAX
    assert R.z_scores(replica_means(case, samples), case.want[0])[2][2] > R.Z_MAX          # as the public call is held to it


@pytest.mark.parametrize("route", ["emulator", "oracle"])
def test_a_flipped_entry_in_lights_drops_half_of_the_samples(route, queries, emu, oracle):
    """property B: the dropped share within 4 binomial SE of 1/2, the mean within 4 SE of the closed form"""
    case = R.property_b()
    samples = emu_samples(case, queries, emu) if route == "emulator" else oracle_samples(case, oracle)
    x = samples[..., :3].reshape(-1, 3)
    n, dropped = len(x), R.clean(x)[1]
    print(f"\n   {dropped} of {n} samples dropped")
    assert abs(dropped / n - 0.5) <= R.Z_MAX * 0.5 / math.sqrt(n)
    report(case.name, "samples", case.check_samples(samples, route))
    report(case.name, "replica means", case.check_means(replica_means(case, samples), route))
    # the bare entry drops nothing
    bare = R.rect_rays(50, R.PDF)
    owner, desc = bare.scene()
    assert np.isfinite(queries.radiance_samples(desc, bare.items[:8], **dict(bare.kw, samples_per_ray=256))[0]).all()
