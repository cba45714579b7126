"""Specular guides on the CPU: vk_trace.h guide_sample (through tests/emu/emu_guides.cpp, on the tree as handed over, the kernel instance
chosen as the launcher chooses it) against tests/guides_ref.py, per sample and with no sample left out: the draw-free decisions (coverage,
the number of continuations, the medium rule) exactly, and the values bit for bit (the device comparison of tests/test_guides_gpu.py
uses the tolerances tests/test_aov_emu.py has for the same quantities: normal and albedo atol 1e-4, depth rtol 1e-5).  Also the reference's own self-tests against closed forms, the window
aggregation bit for bit, and max_bounces = 0 against the first-hit emulator bit for bit.  tests/test_guides_gpu.py runs the same
comparison on the device and takes its scenes from here.  Run with -s for the largest differences per channel."""
import numpy as np
import pytest

import aov_ref
import guides_ref
import special_scenes
import test_aov_emu as aov_shared
from descs import Desc, camera, params
from test_fuzz_scenes import Gen
from vecchio_amd import ffi

f32 = np.float32
W, H = 24, 16
SAMPLES = (0, 1)
BUILDERS = ("random_spheres_iow", "random_spheres_demo", "cornell_box", "final_scene")
FUZZ_SEEDS = (0, 3, 5, 24)


@pytest.fixture(scope="session")
def emu_guides(built):
    import emu_guides_ffi
    emu_guides_ffi.load()
    return emu_guides_ffi


# ---------------------------------------------------------------- hand-built scenes (shared with tests/test_guides_gpu.py)
def _sky(w=W, h=H, seed=5):
    return params(w, h, 1, seed=seed, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SKY)


def mirror_facing_mirror():
    """two parallel mirrors with the camera between them: the bounce cap is reached"""
    d = Desc()
    m1 = d.mat(ffi.VK_MAT_METAL, d.solid(0.9, 0.8, 0.7), 0.0)
    m2 = d.mat(ffi.VK_MAT_METAL, d.solid(0.7, 0.8, 0.9), 0.0)
    world = special_scenes._bvh_chain(d, [d.xy_rect(-50, 50, -50, 50, -3.0, m1), d.xy_rect(-50, 50, -50, 50, 3.0, m2),
                                          d.sphere((0.8, 0.3, -1.5), 0.4, d.lambertian(0.2, 0.6, 0.3))])
    return d, d.finish(world), camera((0, 0, 0), (0.1, 0.05, -1), vfov=50.0, aspect=W / H), _sky()


def glass_before_checker():
    d = Desc()
    chk = d.mat(ffi.VK_MAT_LAMBERTIAN, d.checker(d.solid(0.1, 0.2, 0.3), d.solid(0.9, 0.8, 0.7)))
    world = special_scenes._bvh_chain(d, [d.sphere((0, 0, 0), 1.0, d.mat(ffi.VK_MAT_DIELECTRIC, 0, 1.5)),
                                          d.xy_rect(-30, 30, -30, 30, -4.0, chk), d.xz_rect(-30, 30, -30, 30, -1.3, chk)])
    return d, d.finish(world), camera((0, 0.5, 5), (0, 0, 0), vfov=35.0, aspect=W / H, aperture=0.1, focus=5.0), _sky()


def glass_and_media():
    """a glass ball inside a ball of fog, and a ball of fog behind a glass pane: media met on continuation segments draw from the
    continuation stream"""
    d = Desc()
    glass = d.mat(ffi.VK_MAT_DIELECTRIC, 0, 1.5)
    fog_a = d.medium(d.sphere((-2.2, 0, 0), 1.8, d.lambertian(0.5, 0.5, 0.5)), 0.5, d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(0.8, 0.2, 0.2)))
    ball = d.sphere((-2.2, 0, 0), 0.8, glass)
    pane = d.boxy((0.8, -1.5, 1.0), (3.8, 1.5, 1.3), glass)
    fog_b = d.medium(d.sphere((2.2, 0, -1.5), 1.4, d.lambertian(0.5, 0.5, 0.5)), 0.7, d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(0.2, 0.3, 0.9)))
    wall = d.xy_rect(-30, 30, -30, 30, -5.0, d.lambertian(0.6, 0.6, 0.5))
    world = special_scenes._bvh_chain(d, [fog_a, ball, pane, fog_b, wall])
    return d, d.finish(world), camera((0, 0.3, 9), (0, 0, 0), vfov=40.0, aspect=W / H), _sky(seed=11)


def rough_metal():
    """a Metal of fuzz 0.3 beside one of fuzz 0: fuzz_max decides which is a mirror"""
    d = Desc()
    world = special_scenes._bvh_chain(d, [d.sphere((-1.1, 0, 0), 1.0, d.mat(ffi.VK_MAT_METAL, d.solid(0.8, 0.6, 0.2), 0.3)),
                                          d.sphere((1.1, 0, 0), 1.0, d.mat(ffi.VK_MAT_METAL, d.solid(0.8, 0.8, 0.8), 0.0)),
                                          d.sphere((0, -101, 0), 100.0, d.lambertian(0.5, 0.5, 0.5))])
    return d, d.finish(world), camera((0, 1, 6), (0, 0, 0), vfov=35.0, aspect=W / H), _sky()


def moving_sphere_in_mirror():
    d = Desc()
    mirror = d.xy_rect(-6, 6, -4, 4, -3.0, d.mat(ffi.VK_MAT_METAL, d.solid(0.95, 0.95, 0.95), 0.0))
    mover = d.moving_sphere((-1.5, 0, 2.0), (1.5, 0.8, 2.0), 0.0, 1.0, 0.7, d.lambertian(0.8, 0.3, 0.1))
    world = special_scenes._bvh_chain(d, [mirror, mover])
    return d, d.finish(world), camera((0, 2.5, 4.5), (0, 0, -3), vfov=50.0, aspect=W / H, t0=0.0, t1=1.0), _sky(seed=3)


def camera_inside_glass():
    d = Desc()
    world = special_scenes._bvh_chain(d, [d.sphere((0, 0, 0), 2.0, d.mat(ffi.VK_MAT_DIELECTRIC, 0, 1.5)),
                                          d.sphere((0, 0, -6), 1.5, d.lambertian(0.7, 0.2, 0.2)),
                                          d.sphere((0, -103, 0), 100.0, d.lambertian(0.3, 0.5, 0.3))])
    return d, d.finish(world), camera((0.3, 0.2, 0.5), (0, 0, -6), vfov=70.0, aspect=W / H), _sky()


HAND_BUILT = {"mirror_facing_mirror": mirror_facing_mirror, "glass_before_checker": glass_before_checker,
              "glass_and_media": glass_and_media, "rough_metal": rough_metal, "moving_sphere_in_mirror": moving_sphere_in_mirror,
              "camera_inside_glass": camera_inside_glass}


def builder(host_scenes, name):
    hs, cam = host_scenes(name)
    return hs.desc, cam, hs.params(W, 1, 50, seed=7, height=H)


_FUZZ = {}


def fuzz(seed):
    """(the generator owns the arrays the description points into, image texels among them: it is kept)"""
    if seed not in _FUZZ:
        g = Gen(1000 + seed)
        _FUZZ[seed] = (g,) + tuple(g.build())
    return _FUZZ[seed][1:]


# ---------------------------------------------------------------- comparison (shared with tests/test_guides_gpu.py)
class Worst(aov_shared.Worst):
    pass


def check_per_sample(got, ref, p, worst=None, exact=False):
    """every sample of every pixel: `got` (single-sample results, one per sample of `ref`) against the reference.  Exact: coverage, the
    number of continuations, which samples are dropped, the zero normal of a medium or a miss.  Values: bit for bit when `exact` (the
    emulator: the reference restates its arithmetic operation by operation, so a wrong tint order or a missing tint shows), otherwise
    (the device) the tolerances of test_aov_emu.check_per_sample for the same quantities."""
    for k, g in enumerate(got):
        dropped = ref["dropped"][k]
        kept_hit = (ref["coverage"][k] == 1) & ~dropped
        np.testing.assert_array_equal(g["coverage"] == 1, kept_hit)
        np.testing.assert_array_equal(g["bounces"][~dropped], ref["bounces"][k][~dropped])
        if "dropped" in g:
            np.testing.assert_array_equal(g["dropped"], dropped)
        kept = ~dropped
        if exact:
            for ch in ("normal", "albedo"):
                np.testing.assert_array_equal(g[ch][kept].view(np.uint32), ref[ch][k][kept].view(np.uint32), err_msg=ch)
            np.testing.assert_array_equal(g["depth"][kept_hit].view(np.uint32), ref["depth"][k][kept_hit].view(np.uint32))
        np.testing.assert_allclose(g["normal"][kept], ref["normal"][k][kept], atol=1e-4)
        np.testing.assert_allclose(g["albedo"][kept], ref["albedo"][k][kept], atol=1e-4)
        np.testing.assert_allclose(g["depth"][kept_hit], ref["depth"][k][kept_hit], rtol=1e-5)
        assert np.isposinf(g["depth"][~kept_hit]).all()
        zero = kept & (ref["normal"][k] == 0).all(-1)
        assert (g["normal"][zero] == 0).all()
        if worst is not None:
            sub = {ch: np.where(kept[..., None] if g[ch].ndim == 3 else kept, g[ch], ref[ch][k]) for ch in aov_ref.CHANNELS}
            worst.add(sub, ref, k)


def run(oracle, emu_guides, desc, cam, p, samples=SAMPLES, max_bounces=4, fuzz_max=0.0):
    ref = guides_ref.ref_guides(oracle, desc, cam, p, samples, max_bounces, fuzz_max)
    got, features = emu_guides.guide_samples(desc, cam, p, samples[0], len(samples), max_bounces, fuzz_max)
    w = Worst()
    check_per_sample(got, ref, p, w, exact=True)
    print("\n   emulator vs reference:", w, " delta samples %d, mean bounces %.3f, dropped %d" % (
        int(ref["delta"].sum()), float(ref["bounces"].mean()), int(ref["dropped"].sum())))
    return ref, got, features


# ---------------------------------------------------------------- self-tests of the reference against closed forms
def test_ref_mirror_plane_depth_is_the_sum_of_the_two_legs(oracle):
    d = Desc()
    mirror = d.xz_rect(-50, 50, -50, 50, 0.0, d.mat(ffi.VK_MAT_METAL, d.solid(0.5, 1.0, 0.25), 0.0))
    wall = d.xy_rect(-50, 50, 0, 50, -6.0, d.lambertian(0.8, 0.4, 0.2))
    desc = d.finish(d.big_box(mirror, wall))
    cam = camera((0, 2, 0), (0, 0, -3), vfov=20.0)
    p = params(6, 6, 1, seed=1, integrator=ffi.VK_INTEGRATOR_SCATTER)
    ref = guides_ref.ref_guides(oracle, desc, cam, p, [0])
    assert ref["delta"].all() and (ref["bounces"] == 1).all()
    for y in range(6):
        for x in range(6):
            o, dd, _ = aov_ref.primary_ray(oracle, cam, p, x, y, 0)
            o, dd = o.astype(np.float64), dd.astype(np.float64)
            u = dd / np.linalg.norm(dd)
            leg1 = -o[1] / u[1]                                   # down to y = 0
            hit = o + leg1 * u
            r = u * np.array([1.0, -1.0, 1.0])                    # mirrored in the plane
            leg2 = (-6.0 - hit[2]) / r[2]
            np.testing.assert_allclose(ref["depth"][0, y, x], leg1 + leg2, rtol=1e-5)
            np.testing.assert_allclose(ref["normal"][0, y, x], [0, 0, 1], atol=1e-6)
            np.testing.assert_allclose(ref["albedo"][0, y, x], np.float32([0.5, 1.0, 0.25]) * np.float32([0.8, 0.4, 0.2]), rtol=1e-6)
    # the virtual image of a planar mirror: the same depth as the wall's mirror image seen directly
    np.testing.assert_array_equal(ref["first"]["albedo"][0], np.broadcast_to(f32([0.5, 1.0, 0.25]), (6, 6, 3)))


def test_ref_glass_slab_exit_is_parallel_to_entry(oracle):
    d = Desc()
    slab = d.boxy((-20, -20, -1.0), (20, 20, 0.0), d.mat(ffi.VK_MAT_DIELECTRIC, 0, 1.5))
    wall = d.xy_rect(-50, 50, -50, 50, -5.0, d.lambertian(0.3, 0.6, 0.9))
    desc = d.finish(d.big_box(slab, wall))
    cam = camera((1, 2, 4), (0, 0, -1), vfov=25.0)
    p = params(5, 5, 1, seed=2, integrator=ffi.VK_INTEGRATOR_SCATTER)
    fh = oracle.first_hits(desc, cam, p, 0, 1)[:, :, 0]
    phase = guides_ref.phase_materials(desc.contents)
    for y in range(5):
        for x in range(5):
            r = fh[y, x]
            rec = dict(p=r["p"], normal=r["normal"], t=r["t"], u=r["u"], v=r["v"], front=bool(r["front"]), material=int(r["material"]),
                       medium=False)
            a, n, dep, b, trail = guides_ref.follow(oracle, desc, p, y * 5 + x, 0, rec, r["direction"], r["time"], 4, 0.0, phase)
            assert b == 2 and [t["kind"] for t in trail] == ["refract", "refract"]
            u_in = r["direction"] / np.linalg.norm(r["direction"])
            u_out = trail[1]["direction"] / np.linalg.norm(trail[1]["direction"])
            np.testing.assert_allclose(u_out, u_in, atol=2e-6)
            inside = trail[0]["direction"] / np.linalg.norm(trail[0]["direction"])
            # Snell: sin(inside) = sin(outside) / 1.5 about the z axis
            np.testing.assert_allclose(np.hypot(inside[0], inside[1]), np.hypot(u_in[0], u_in[1]) / 1.5, atol=2e-6)
            np.testing.assert_allclose(a, [0.3, 0.6, 0.9], rtol=1e-6)
            np.testing.assert_allclose(n, [0, 0, 1], atol=0)


def test_ref_total_internal_reflection_inside_a_sphere(oracle):
    d = Desc()
    desc = d.finish(d.big_box(d.sphere((0, 0, 0), 1.0, d.mat(ffi.VK_MAT_DIELECTRIC, 0, 1.5)),
                              d.sphere((0, 0, -50), 1.0, d.lambertian(0.5, 0.5, 0.5))))
    p = params(4, 4, 1, seed=1, integrator=ffi.VK_INTEGRATOR_SCATTER)
    phase = guides_ref.phase_materials(desc.contents)
    # a chord from inside that meets the surface at 60 degrees from the normal: beyond the critical angle asin(1/1.5) = 41.8 degrees
    s60 = np.sin(np.radians(60.0))
    origin = [float(s60), 0.0, 0.4]
    h = oracle.hit(desc, origin, [0.0, 0.0, -1.0], 0.0, 0.001, float("inf"), 0)
    assert h is not None and not h["front"]
    np.testing.assert_allclose(h["p"], [s60, 0, -0.5], atol=1e-6)
    nd, tir = guides_ref.dielectric_direction(f32([0, 0, -1]), f32(h["normal"]), h["front"], 1.5)
    assert tir
    np.testing.assert_allclose(nd, guides_ref.reflect(f32([0, 0, -1]), f32(h["normal"])), atol=0)
    # the reflected chord keeps the angle: every further meeting is total internal reflection again, so the cap ends the walk
    rec = dict(p=f32(h["p"]), normal=f32(h["normal"]), t=f32(h["t"]), u=f32(h["u"]), v=f32(h["v"]), front=False, material=h["material"],
               medium=False)
    a, n, dep, b, trail = guides_ref.follow(oracle, desc, p, 0, 0, rec, f32([0, 0, -1]), 0.0, 8, 0.0, phase)
    assert b == 8 and all(t["kind"] == "tir" for t in trail)
    chord = 2 * np.cos(np.radians(60.0))
    np.testing.assert_allclose(dep, 0.9 + 8 * chord, rtol=1e-5)
    # ... and at 30 degrees it leaves
    origin = [0.5, 0.0, 0.5]
    h = oracle.hit(desc, origin, [0.0, 0.0, -1.0], 0.0, 0.001, float("inf"), 0)
    nd, tir = guides_ref.dielectric_direction(f32([0, 0, -1]), f32(h["normal"]), h["front"], 1.5)
    assert not tir and np.isfinite(nd).all()


def test_segment_seed_wraps():
    assert guides_ref.segment_seed(0, 0, 0, 1) == guides_ref.GOLDEN
    assert guides_ref.segment_seed(2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 8) < 2 ** 64


# ---------------------------------------------------------------- the emulator against the reference
@pytest.mark.parametrize("name", BUILDERS)
def test_builder_scene_per_sample(name, oracle, emu_guides, host_scenes):
    desc, cam, p = builder(host_scenes, name)
    ref, _, _ = run(oracle, emu_guides, desc, cam, p)
    assert ref["delta"].any() and ref["bounces"].max() >= 1, "the frame must show a delta hit"


@pytest.mark.parametrize("name", sorted(HAND_BUILT))
def test_hand_built_scene_per_sample(name, oracle, emu_guides):
    d, desc, cam, p = HAND_BUILT[name]()
    ref, got, _ = run(oracle, emu_guides, desc, cam, p)
    assert ref["delta"].any()
    if name == "mirror_facing_mirror":
        assert (ref["bounces"] == 4).any(), "the bounce cap must be reached"
    if name == "glass_and_media":
        later_medium = (ref["bounces"] >= 1) & (ref["normal"] == 0).all(-1) & (ref["coverage"] == 1)
        assert later_medium.any(), "a medium must be the terminal surface of a continuation"
    if name == "moving_sphere_in_mirror":
        assert ((ref["bounces"] == 1) & (np.abs(ref["albedo"] - f32([0.95 * 0.8, 0.95 * 0.3, 0.95 * 0.1])).max(-1) < 1e-3)).any()
    if name == "camera_inside_glass":
        assert (ref["bounces"] >= 1).all()


@pytest.mark.parametrize("fuzz_max", [0.0, 0.5])
def test_fuzz_max_decides_what_is_a_mirror(fuzz_max, oracle, emu_guides):
    d, desc, cam, p = rough_metal()
    ref, _, _ = run(oracle, emu_guides, desc, cam, p, fuzz_max=fuzz_max)
    rough = ref["first"]["material"] == 0                      # the fuzz-0.3 sphere's material is the first one made
    seen = rough & (ref["first"]["coverage"] == 1)
    assert seen.any()
    assert (ref["bounces"][seen] >= 1).all() if fuzz_max >= 0.3 else (ref["bounces"][seen] == 0).all()


def test_bounce_cap_of_eight(oracle, emu_guides):
    d, desc, cam, p = mirror_facing_mirror()
    p.width, p.height = 12, 8
    ref, _, _ = run(oracle, emu_guides, desc, cam, p, samples=(0,), max_bounces=8)
    assert (ref["bounces"] == 8).any()


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_graph_per_sample(seed, oracle, emu_guides):
    desc, cam, p = fuzz(seed)
    run(oracle, emu_guides, desc, cam, p)


def bits_equal(got, want, channels):
    for ch in channels:
        np.testing.assert_array_equal(got[ch].view(np.uint32), want[ch].view(np.uint32), err_msg=ch)


def test_windows_aggregate_exactly(emu_guides, host_scenes):
    for name in ("random_spheres_iow", "cornell_box"):
        desc, cam, p = builder(host_scenes, name)
        one, _ = emu_guides.guide_samples(desc, cam, p, 0, 12)
        for lo, hi in ((0, 8), (4, 12)):
            bits_equal(emu_guides.guide_window(desc, cam, p, lo, hi - lo), guides_ref.aggregate(one[lo:hi]), guides_ref.CHANNELS)
    d, desc, cam, p = glass_and_media()
    one, _ = emu_guides.guide_samples(desc, cam, p, 3, 7)
    bits_equal(emu_guides.guide_window(desc, cam, p, 3, 7), guides_ref.aggregate(one), guides_ref.CHANNELS)


def test_zero_bounces_is_the_first_hit_emulator_bit_for_bit(emu, emu_guides, host_scenes):
    cases = [builder(host_scenes, n) for n in BUILDERS] + [HAND_BUILT[n]()[1:] for n in sorted(HAND_BUILT)]
    d, desc, cam, p = aov_shared.dropped_checker()
    cases.append((desc, cam, p))
    for desc, cam, p in cases:
        got = emu_guides.guide_window(desc, cam, p, 2, 3, max_bounces=0)
        bits_equal(got, emu.aov_window(desc, cam, p, 2, 3), aov_ref.CHANNELS)
        assert (got["bounces"] == 0).all()
