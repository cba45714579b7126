"""The scattering and light-sampling laws on the CPU: what one bounce of vk_trace.h shade_hit (the shade emulator) DRAWS, against the f64
closed forms of tests/scatter_laws_ref.py — the distribution of the scattered direction and the weight it carries, which no
expectation of tests/test_radiometry.py can see (mixture weights 0.25 / 0.75 in value AND generate leave every mean where it was).

First the closed forms themselves against f64 numpy sampling (default_rng) or quadrature of the law, so that the module is a reference;
then every case on the emulator: statistics, identities, power controls, the exclusion cap; then the traced pair, whose hit records the
library's own walk writes (tests/emu/emu_rays.cpp), which ties the hand-made records' conventions to it.
tests/test_gpu_scatter_laws.py holds the device to the same cases.  pytest -s prints every case's summary."""
import math

import numpy as np
import pytest

import scatter_laws_ref as L
from shade_ref import assert_shaded_equal

f64 = np.float64
M = 400_000                # f64 samples of a self-test: SE 1.6e-3 of a unit-variance quantity


@pytest.fixture(scope="module")
def emu_shade(built):
    import emu_shade_ffi
    emu_shade_ffi.load()
    return emu_shade_ffi


@pytest.fixture(scope="module")
def emu_queries(built):
    import emu_queries_ffi
    emu_queries_ffi.load()
    return emu_queries_ffi


# ================================================================ the closed forms are a reference
def _ball(rng, m):
    """uniform in the unit ball as util.rs:31-39 makes it: rejection from the cube"""
    p = rng.uniform(-1.0, 1.0, (2 * m, 3))
    return p[(p * p).sum(1) < 1.0][:m]


def _sphere(rng, m):
    """uniform on the unit sphere as material.rs:51-58 makes it"""
    a, z = rng.uniform(0.0, 2.0 * math.pi, m), rng.uniform(-1.0, 1.0, m)
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(a), r * np.sin(a), z], 1)


def _within(got, want, se, what):
    assert abs(got - want) <= L.Z_MAX * se, f"{what}: {got} want {want} se {se}"


def test_cap_share_against_sampling():
    rng = np.random.default_rng(1)
    n = np.array([0.0, 1.0, 0.0])
    mirror = L.reflect(L.unit(np.array(L._incoming(0.2, 1.7))), n)
    assert abs(mirror @ n - 0.2) < 1e-12
    want, wrong = L.cap_share(0.5, 0.2), L.cap_share_surface(0.5, 0.2)
    assert abs(want - 0.216) < 1e-12 and abs(wrong - 0.3) < 1e-12
    for draw, p in ((_ball, want), (_sphere, wrong)):
        below = ((mirror + 0.5 * draw(rng, M)) @ n <= 0.0).mean()
        _within(below, p, math.sqrt(p * (1 - p) / M), draw.__name__)


def test_cos2_of_normal_plus_sphere_is_uniform():
    rng = np.random.default_rng(2)
    n = L.unit(np.array([0.3, -0.5, 0.8]))
    c2 = (L.unit(n + _sphere(rng, M)) @ n) ** 2
    _within(c2.mean(), 1 / 2, c2.std() / math.sqrt(M), "mean")
    _within((c2 * c2).mean(), 1 / 3, (c2 * c2).std() / math.sqrt(M), "second moment")
    hist = np.histogram(c2, 16, (0.0, 1.0))[0] / M
    assert np.abs(hist - 1 / 16).max() <= L.Z_MAX * math.sqrt(15 / 256 / M) * 1.25        # (16 bins: a little room for the largest)


@pytest.mark.parametrize("rect", [L.RECT] + L.ZOO_RECTS + L.ZOO_BOX.plain, ids=lambda r: f"axes{r.axes}")
def test_rect_pdf_integrates_to_one(rect):
    """int light(d) d omega over the rect's solid angle, d omega = cos / r^2 dA by midpoint quadrature over the rect, for directions of
    any length (pdf_value is a function of the direction, not of its length)"""
    o = np.array([0.3, -0.2, 0.1])
    m = 300
    a0, a1, a2 = rect.axes
    q = np.zeros((m * m, 3))
    ga = rect.c0 + (np.arange(m) + 0.5) * (rect.c1 - rect.c0) / m
    gb = rect.d0 + (np.arange(m) + 0.5) * (rect.d1 - rect.d0) / m
    q[:, a0], q[:, a1], q[:, a2] = np.repeat(ga, m), np.tile(gb, m), rect.k
    v = q - o
    r2 = (v * v).sum(1)
    scale = np.random.default_rng(3).uniform(0.3, 3.0, m * m)
    value, _ = rect.pdf(o, v * scale[:, None])
    d_omega = np.abs(v[:, a2]) / np.sqrt(r2) / r2 * rect.area / (m * m)
    assert abs((value * d_omega).sum() - 1.0) < 1e-9
    assert not rect.pdf(o, -v)[0].any()                                 # behind the origin: t < 0.001


def test_cone_pdf_integrates_to_one():
    """int light(d) d omega over the directions that meet the sphere, in (z, phi) about the axis: d omega = dz dphi.  The quadrature's
    error is one ring of cells at the cone's rim: 1 / m of the cone"""
    o = np.array(L.P_SPHERE, f64)
    sph = L.SPHERE_OVER
    w = L.unit(sph.center - o)
    t1, t2 = L.tangents(w)
    cm = sph.cos_max(o)
    m, k = 4000, 16
    z = (cm - 0.02) + (np.arange(m) + 0.5) * (1.0 - cm + 0.02) / m
    phi = (np.arange(k) + 0.5) * 2.0 * math.pi / k
    zz, pp = np.repeat(z, k), np.tile(phi, m)
    s = np.sqrt(1.0 - zz * zz)
    d = zz[:, None] * w + (s * np.cos(pp))[:, None] * t1 + (s * np.sin(pp))[:, None] * t2
    value, _ = sph.pdf(o, 1.7 * d)
    total = value.sum() * ((1.0 - cm + 0.02) / m) * (2.0 * math.pi / k)
    assert abs(total - 1.0) < 2.0 / (m * (1.0 - cm) / (1.0 - cm + 0.02))


def test_ball_moments():
    b = _ball(np.random.default_rng(4), M)
    r3 = (b * b).sum(1) ** 1.5
    _within((b[:, 0] ** 2).mean(), L.BALL_X2, (b[:, 0] ** 2).std() / math.sqrt(M), "E x^2")
    _within(r3.mean(), L.BALL_R3, r3.std() / math.sqrt(M), "E r^3")
    s = _sphere(np.random.default_rng(5), M)
    _within((s[:, 0] ** 2).mean(), L.SPHERE_X2, (s[:, 0] ** 2).std() / math.sqrt(M), "sphere E x^2")


def test_cone_moments():
    cm = L.SPHERE_AWAY.cos_max(np.array(L.P_SPHERE, f64))
    z = np.random.default_rng(6).uniform(cm, 1.0, M)
    ez, var, e_lin, e_root = L.cone_moments(cm)
    for x, want, what in ((z, ez, "E z"), ((z - ez) ** 2, var, "Var z"), (1 - z * z, e_lin, "E (1 - z^2)"), (np.sqrt(1 - z * z), e_root, "E sqrt")):
        _within(x.mean(), want, x.std() / math.sqrt(M), what)
    assert e_root > 2.0 * e_lin                                          # (the control is far from the law)


def test_cosine_density_moments():
    """util.rs:52-63 in f64: E cos = 2/3, E cos^2 = 1/2"""
    rng = np.random.default_rng(7)
    z = np.sqrt(1.0 - rng.uniform(0.0, 1.0, M))
    _within(z.mean(), 2 / 3, z.std() / math.sqrt(M), "E cos")
    _within((z * z).mean(), 1 / 2, (z * z).std() / math.sqrt(M), "E cos^2")


def test_the_case_list():
    """what the issue lists is there, N is the issue's, every light point is farther than 1.5 and every plane of the zoo has a
    coordinate of its own"""
    assert L.N == 65536 and len(L.CASES) == 34
    for p, lights in ((L.P_RECT, [L.RECT]), (L.P_ZOO, L.ZOO_RECTS + L.ZOO_BOX.plain)):
        for r in lights:
            a0, a1, a2 = r.axes
            near = np.zeros(3)
            near[a0], near[a1], near[a2] = np.clip(p[a0], r.c0, r.c1), np.clip(p[a1], r.d0, r.d1), r.k
            assert np.linalg.norm(near - np.array(p)) > 1.5
    planes = [(r.axes[2], r.k) for r in L.ZOO_RECTS + L.ZOO_BOX.plain] + [(2, -7.0), (1, 2.0), (0, 1.5), (1, 3.5)]
    assert len(set(planes)) == len(planes)
    assert (len(L.interleaved(["lambertian-pdf-rect"], 256)[0])) % 256 != 0
    xs = [abs(n[0]) for n in L.ONB_NORMALS]
    assert sum(x > 0.9 for x in xs) == 3 and 0.8 < min(xs) <= 0.9


# ================================================================ every case on the emulator
@pytest.mark.parametrize("name", list(L.CASES))
def test_case_on_the_emulator(name, emu_shade):
    case = L.CASES[name]
    owner, desc = case.scene.desc()
    rays, hits, states = case.items()
    out = emu_shade.shade_hits(desc, rays, hits, states, **case.kwargs())
    report = case.check(out, rays, hits, states)
    print(f"\n   {report.summary()}", end="")
    report.finish()


# ================================================================ the traced pair
@pytest.mark.parametrize("which", list(L.TRACED))
def test_traced_pair_on_the_emulator(which, emu_shade, emu_queries):
    """the same laws on records the walk writes: rays aimed at a real floor.  The records must be what the hand-made ones assume: a hit,
    the floor's material, front, the normal +y (oriented against the ray), p on the floor"""
    scene, integrator, seed, law = L.TRACED[which]
    case = L.CASES[law]
    owner, desc = L.SCENES[scene].desc()
    rays = L.traced_rays(which)
    hits, _ = emu_queries.trace_rays(desc, rays)
    assert (hits["hit"] == 1).all() and (hits["front"] == 1).all() and (hits["material"] == case.material).all()
    assert (hits["normal"] == np.float32([0, 1, 0])).all() and np.abs(hits["t"] - 1.0).max() < 1e-5
    states = L.make_path_states(len(rays), seed)
    out = emu_shade.shade_hits(desc, rays, hits, states, **case.kwargs())
    report = case.check(out, rays, hits, states)
    print(f"\n   traced {report.summary()}", end="")
    report.finish()


def test_an_interleaved_batch_is_its_cases(emu_shade):
    """an item's result depends on the item alone: a small interleaved batch, un-permuted, is each case's own results"""
    names = L.batches()[("rect", L.PDF)]
    owner, desc = L.SCENES["rect"].desc()
    rays, hits, states, perm, slices = L.interleaved(names, 512)
    kw = L.CASES[names[0]].kwargs()
    out = L.unpermute(emu_shade.shade_hits(desc, rays, hits, states, **kw), perm)
    for name in names:
        r, h, s = L.CASES[name].items(512)
        alone = emu_shade.shade_hits(desc, r, h, s, **kw)
        assert_shaded_equal(out[slices[name]], alone, name)
    L.check_misses(out[slices[None]], L.unpermute(states, perm)[slices[None]])
