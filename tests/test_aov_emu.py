"""First-hit buffers on the CPU: vk_trace.h aov_sample (through tests/emu, on the tree as handed over, the kernel instance chosen as
vk_api.hip enqueue_aov chooses it) against reference (a) of tests/aov_ref.py, per sample and with no sample left out, on every scene
the emulator parity tests use, media included: a medium's distance is drawn from the radiance sample's own stream, after the camera's
draws, so sample s has the first hit radiance sample s has.  Also: the oracle's primary rays against a numpy restatement of the camera
draws, the window aggregation rule (dropped samples included) bit for bit, and the scenes the GPU module shares (SCENES, dropped_*).

Tolerances are those tests/test_gpu_aov.py uses between device and oracle (normal and albedo atol 1e-4, depth rtol 1e-5); coverage, the
medium rule and the miss rule are exact.  Run with -s to see the largest difference per channel."""
import ctypes as C

import numpy as np
import pytest

import aov_ref
import special_scenes
from descs import Desc, camera, params
from test_emu_parity import BUILDER_SCENES
from test_fuzz_scenes import Gen
from vecchio_amd import ffi

f32 = np.float32
FUZZ_SEEDS = tuple(range(32))
SIZE = 32                        # builder and special scenes: SIZE x SIZE pixels (the fuzz graphs keep their 20 x 16)
SAMPLES = tuple(range(8))        # eight samples per pixel: what the sparsest media graph (seed 24) needs to show a medium hit
# Gen(1001)'s only medium lies outside its camera's view: no primary ray reaches it at any size (test_the_unseen_medium_is_unseen), so
# that graph is compared per sample like every other but cannot show a medium hit
UNSEEN_MEDIA = (1,)


# ---------------------------------------------------------------- scenes shared with tests/test_gpu_aov.py
def fog_scene():
    """a ball of fog in front of an emitting wall: a ray ends in the fog or on the wall, by the sample's own draw"""
    d = Desc()
    emit = (0.3, 0.6, 0.9)
    back = d.xy_rect(-20, 20, -20, 20, -5.0, d.light(*emit))
    fog = d.medium(d.sphere((0, 0, 0), 2.0, d.lambertian(0.5, 0.5, 0.5)), 0.4, d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(0.8, 0.2, 0.2)))
    world = d.big_box(fog, back)
    return d, d.finish(world), emit


def fog():
    d, desc, _ = fog_scene()
    return d, desc, camera((0, 0, 10), (0, 0, 0), vfov=30.0), params(16, 16, 2, max_depth=1, seed=11, integrator=ffi.VK_INTEGRATOR_SCATTER)


def camera_inside_medium():
    """the camera (with a lens) inside a medium of checkered phase function, surfaces inside and outside it, a second medium behind"""
    d = Desc()
    chk = d.checker(d.solid(0.9, 0.1, 0.1), d.solid(0.1, 0.9, 0.1))
    outer = d.medium(d.sphere((0, 0, 0), 4.0, d.mat(ffi.VK_MAT_DIELECTRIC, 0, 1.5)), 0.25, d.mat(ffi.VK_MAT_ISOTROPIC, chk))
    inner = d.sphere((0.5, 0.2, -2.0), 0.7, d.lambertian(0.2, 0.3, 0.8))
    far = d.translate(d.medium(d.boxy((-1, -1, -1), (1, 1, 1), d.lambertian(1, 1, 1)), 0.8, d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(0.6, 0.6, 0.1))),
                      (-1.5, 0.5, -6.5))
    wall = d.xy_rect(-30, 30, -30, 30, -9.0, d.lambertian(0.5, 0.5, 0.5))
    world = d.big_box(d.big_box(outer, inner), d.big_box(far, wall))
    desc = d.finish(world)
    cam = camera((0, 0, 1), (0, 0, -5), vfov=70.0, aperture=0.4, focus=3.0)
    return d, desc, cam, params(16, 16, 2, seed=5, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SKY)


def dropped_spheres():
    """spheres only (the lean kernel instance): Lambertian spheres whose solid colour has a NaN or an infinite component among finite
    ones, seen through a wide lens far out of focus, so that the samples of one pixel land on different spheres"""
    d = Desc()
    nan, inf = float("nan"), float("inf")
    cols = [(0.7, 0.2, 0.2), (nan, 0.5, 0.5), (0.2, 0.7, 0.2), (0.5, inf, 0.5), (0.2, 0.2, 0.7), (0.5, 0.5, -inf)]
    refs = [d.sphere((0, -1000.5, 0), 1000.0, d.lambertian(0.5, 0.5, 0.5))]
    for i in range(-2, 3):
        for j in range(-2, 3):
            refs.append(d.sphere((1.1 * i, 0.0, 1.1 * j), 0.5, d.lambertian(*cols[(3 * i + j) % len(cols)])))
    world = special_scenes._bvh_chain(d, refs)
    desc = d.finish(world)
    cam = camera((3, 4, 5), (0, 0, 0), vfov=40.0, aperture=0.6, focus=3.0)
    return d, desc, cam, params(16, 16, 8, seed=9, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SKY)


def dropped_checker():
    """a mixed scene (the everything instance): a checker with a NaN child on a big sphere, an emitter with an infinite colour behind it
    (clamped to 1: kept), a fog ball whose phase function has a NaN colour (a dropped medium hit)"""
    d = Desc()
    nan, inf = float("nan"), float("inf")
    chk = d.checker(d.solid(0.3, nan, 0.3), d.solid(0.8, 0.8, 0.1))
    ball = d.sphere((0, 0, 0), 2.0, d.mat(ffi.VK_MAT_LAMBERTIAN, chk))
    back = d.xy_rect(-20, 20, -20, 20, -5.0, d.light(inf, 2.0, 0.25))
    fogm = d.medium(d.sphere((2.5, 1.5, 2.0), 1.2, d.lambertian(0.5, 0.5, 0.5)), 0.6, d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(0.5, 0.5, nan)))
    world = d.big_box(d.big_box(ball, fogm), back)
    desc = d.finish(world)
    cam = camera((0, 0, 10), (0, 0, 0), vfov=40.0, aperture=0.3, focus=6.0)
    return d, desc, cam, params(16, 16, 8, seed=13, integrator=ffi.VK_INTEGRATOR_SCATTER)


DROPPED = {"dropped_spheres": dropped_spheres, "dropped_checker": dropped_checker}
EXTRA = {"fog": fog, "camera_inside_medium": camera_inside_medium}


def special(name):
    d, desc, cam, p = special_scenes.ALL[name]()
    p.width, p.height = SIZE, SIZE
    return d, desc, cam, p


def fuzz(seed):
    g = Gen(1000 + seed)
    desc, cam, p = g.build()
    return g, desc, cam, p


# ---------------------------------------------------------------- comparison
class Worst:
    """largest difference seen per channel"""

    def __init__(self):
        self.v = dict(albedo=0.0, normal=0.0, depth_rel=0.0)

    def add(self, got, ref, k):
        hit = ref["coverage"][k] == 1
        with np.errstate(invalid="ignore"):
            self.v["albedo"] = max(self.v["albedo"], float(np.nanmax(np.abs(got["albedo"] - ref["albedo"][k]), initial=0.0)))
            self.v["normal"] = max(self.v["normal"], float(np.nanmax(np.abs(got["normal"] - ref["normal"][k]), initial=0.0)))
            if hit.any():
                rel = np.abs(got["depth"][hit] - ref["depth"][k][hit]) / np.abs(ref["depth"][k][hit])
                self.v["depth_rel"] = max(self.v["depth_rel"], float(np.nanmax(rel, initial=0.0)))

    def __str__(self):
        return "max |d albedo| %.3g  max |d normal| %.3g  max rel d depth %.3g" % (self.v["albedo"], self.v["normal"], self.v["depth_rel"])


def check_per_sample(got, ref, p, worst=None):
    """every sample of every pixel: `got` (a list of single-sample results, one per sample of `ref`) against reference (a)"""
    assert not ref["dropped"].any() and np.isfinite(ref["albedo"]).all()          # nothing left NaN: every sample is compared
    for k, g in enumerate(got):
        np.testing.assert_array_equal(g["coverage"], ref["coverage"][k])
        hit, med = ref["coverage"][k] == 1, ref["medium"][k]
        # a medium hit: covered, normal exactly 0
        assert hit[med].all() and (g["coverage"][med] == 1).all()
        assert (g["normal"][med].view(np.uint32) << 1 == 0).all()
        # a miss: depth +inf, normal 0, the background the radiance sample sees
        assert np.isposinf(g["depth"][~hit]).all() and (g["normal"][~hit] == 0).all()
        np.testing.assert_allclose(g["albedo"][~hit], aov_ref.background(p, ref["direction"][k][~hit]), atol=1e-4)
        np.testing.assert_allclose(g["normal"], ref["normal"][k], atol=1e-4)
        np.testing.assert_allclose(g["depth"][hit], ref["depth"][k][hit], rtol=1e-5)
        np.testing.assert_allclose(g["albedo"], ref["albedo"][k], atol=1e-4)
        if worst is not None:
            worst.add(g, ref, k)


def kinds(ref):
    """per sample and pixel: 0 miss, 1 surface, 2 medium"""
    return (ref["coverage"] == 1).astype(int) + ref["medium"].astype(int)


def run(oracle, emu, desc, cam, p, samples=SAMPLES):
    ref = aov_ref.ref_a(oracle, desc, cam, p, list(samples))
    got, features = emu.aov_samples(desc, cam, p, samples[0], len(samples))
    assert not any(g["dropped"].any() for g in got)
    w = Worst()
    check_per_sample(got, ref, p, w)
    print("\n   emulator vs oracle:", w)
    if desc.contents.n_media > 0 and kinds(ref).max() == 2:
        assert features != 0
    return ref, got, features


def assert_both_kinds_of_hit(ref):
    k = kinds(ref)
    assert (k == 2).any() and (k == 1).any(), "a media scene must show a medium hit and a surface hit"


# ---------------------------------------------------------------- tests
def _cameras():
    return {"pinhole": camera((3, 2, 6), (0, 0, 0), vfov=35.0),
            "lens": camera((3, 2, 6), (0, 0, 0), vfov=35.0, aperture=0.8, focus=4.0),
            "narrow_shutter": camera((3, 2, 6), (0, 0, 0), vfov=35.0, aperture=0.1, focus=4.0, t0=0.25, t1=0.2501)}


@pytest.mark.parametrize("which", ["pinhole", "lens", "narrow_shutter"])
def test_oracle_primary_rays_equal_the_numpy_restatement(which, oracle):
    """oracle_first_hits' ray of (pixel, sample) against aov_ref.primary_ray, which works the same draws out in numpy float32 from the
    bare stream (oracle_draws): origin, direction and time, bit for bit, 12 x 10 pixels x 3 samples"""
    d = Desc()
    desc = d.finish(d.big_box(d.sphere((0, 0, 0), 1.0, d.lambertian(0.5, 0.5, 0.5)), d.sphere((0, -101, 0), 100.0, d.lambertian(0.5, 0.5, 0.5))))
    cam = _cameras()[which]
    assert (cam.lens_radius > 0) == (which != "pinhole")
    p = params(12, 10, 1, seed=21, integrator=ffi.VK_INTEGRATOR_SCATTER)
    first = 5
    fh = oracle.first_hits(desc, cam, p, first, 3)
    n = 0
    for y in range(p.height):
        for x in range(p.width):
            for k in range(3):
                o, dd, t = aov_ref.primary_ray(oracle, cam, p, x, y, first + k)
                r = fh[y, x, k]
                assert np.array_equal(r["origin"].view(np.uint32), o.view(np.uint32)), (x, y, k)
                assert np.array_equal(r["direction"].view(np.uint32), dd.view(np.uint32)), (x, y, k)
                assert f32(r["time"]).view(np.uint32) == f32(t).view(np.uint32), (x, y, k)
                assert cam.time0 <= r["time"] < cam.time1
                n += 1
    assert n == 360
    if which == "lens":
        assert len(np.unique(fh["origin"].reshape(-1, 3), axis=0)) > 300          # the lens draws do move the origin


def test_oracle_first_hit_is_the_radiance_samples_first_hit(oracle):
    """the new entry against the oracle's own radiance, which it must not have moved: with every material an emitter and depth 1 the
    radiance of sample s is the emitter's colour at the first hit (reference (b)); on the fog scene that tells fog from wall"""
    d, desc, cam, p = fog()
    ref = aov_ref.ref_a(oracle, desc, cam, p, [0, 1])
    b = aov_ref.ref_b_albedo(oracle, desc, cam, p)
    np.testing.assert_allclose(ref["albedo"], b, atol=1e-6)
    assert_both_kinds_of_hit(ref)


@pytest.mark.parametrize("name", BUILDER_SCENES)
def test_builder_scene_per_sample(name, oracle, emu, host_scenes):
    hs, cam = host_scenes(name)
    p = hs.params(SIZE, 2, 50, seed=7, height=SIZE)
    ref, _, _ = run(oracle, emu, hs.desc, cam, p)
    if hs.desc.contents.n_media > 0:
        assert_both_kinds_of_hit(ref)


@pytest.mark.parametrize("name", sorted(special_scenes.ALL))
def test_special_scene_per_sample(name, oracle, emu, built):
    d, desc, cam, p = special(name)
    ref, _, _ = run(oracle, emu, desc, cam, p)
    if desc.contents.n_media > 0:
        assert_both_kinds_of_hit(ref)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_graph_per_sample(seed, oracle, emu, built):
    g, desc, cam, p = fuzz(seed)
    ref, _, _ = run(oracle, emu, desc, cam, p)
    if desc.contents.n_media > 0 and seed not in UNSEEN_MEDIA:
        assert_both_kinds_of_hit(ref)


def test_fuzz_graphs_include_media():
    assert sum(fuzz(seed)[1].contents.n_media > 0 and seed not in UNSEEN_MEDIA for seed in FUZZ_SEEDS) >= 8


def test_the_unseen_medium_is_unseen(oracle):
    """the one exemption from "a media scene shows a medium hit" holds for the reason given: at 8 x the pixels and 16 samples none of
    the 163 840 primary samples ends in the medium, and the frame is not empty"""
    for seed in UNSEEN_MEDIA:
        g, desc, cam, p = fuzz(seed)
        assert desc.contents.n_media > 0
        p.width, p.height = 80, 64
        k = kinds(aov_ref.ref_a(oracle, desc, cam, p, list(range(16))))
        assert not (k == 2).any() and (k == 1).sum() > 1000


@pytest.mark.parametrize("name", sorted(EXTRA))
def test_extra_media_scene_per_sample(name, oracle, emu, built):
    d, desc, cam, p = EXTRA[name]()
    ref, _, _ = run(oracle, emu, desc, cam, p, samples=(0, 1, 2, 3))
    assert_both_kinds_of_hit(ref)


def test_the_stream_decides_the_kind_of_hit(oracle, emu, built):
    """what proves that the stream matters: pixels whose two samples differ in kind (one ends in a medium, the other on a surface
    behind or inside it), in the reference and therefore (coverage and the zero normal are exact) in the emulator"""
    mixed = 0
    for make in (fog, camera_inside_medium, lambda: special("media_and_textures")):
        d, desc, cam, p = make()
        ref = aov_ref.ref_a(oracle, desc, cam, p, [0, 1])
        got, _ = emu.aov_samples(desc, cam, p, 0, 2)
        k = kinds(ref)
        differ = ((k[0] == 2) & (k[1] == 1)) | ((k[0] == 1) & (k[1] == 2))
        assert differ.any()
        zero = [(g["normal"] == 0).all(-1) & (g["coverage"] == 1) for g in got]
        assert np.array_equal(zero[0], k[0] == 2) and np.array_equal(zero[1], k[1] == 2)
        mixed += int(differ.sum())
    print("\n   pixels whose two samples differ in kind:", mixed)


def test_both_kernel_instances_are_reached(emu, host_scenes, built):
    hs, cam = host_scenes("random_spheres_iow")
    _, features = emu.aov_samples(hs.desc, cam, hs.params(8, 1, 50, height=8), 0, 1)
    assert features == 0
    hs, cam = host_scenes("cornell_box")
    _, features = emu.aov_samples(hs.desc, cam, hs.params(8, 1, 50, height=8), 0, 1)
    assert features != 0
    d, desc, cam, p = dropped_spheres()
    assert emu.aov_samples(desc, cam, p, 0, 1)[1] == 0
    d, desc, cam, p = dropped_checker()
    assert emu.aov_samples(desc, cam, p, 0, 1)[1] != 0


def bits_equal(got, want):
    for ch in aov_ref.CHANNELS:
        np.testing.assert_array_equal(got[ch].view(np.uint32), want[ch].view(np.uint32), err_msg=ch)


def test_windows_aggregate_exactly(oracle, emu, host_scenes):
    hs, cam = host_scenes("cornell_box")
    p = hs.params(16, 1, 50, seed=7, height=16)
    one, _ = emu.aov_samples(hs.desc, cam, p, 0, 24)
    for lo, hi in ((0, 16), (8, 24)):
        bits_equal(emu.aov_window(hs.desc, cam, p, lo, hi - lo), aov_ref.aggregate(one[lo:hi]))
    d, desc, cam, p = fog()
    one, _ = emu.aov_samples(desc, cam, p, 3, 7)
    bits_equal(emu.aov_window(desc, cam, p, 3, 7), aov_ref.aggregate(one))


def check_dropped_window(name, p, one, window, ref):
    """`one`: single-sample results of samples 0 .. n - 1 (dropped samples as coverage 0 and zeros), `window`: the n-sample call, `ref`:
    reference (a) of the same samples.  The window is the aggregate of the singles bit for bit, the reference drops the samples the
    singles drop, and some pixel has 0 < hits < n because of a drop."""
    n = len(one)
    bits_equal(window, aov_ref.aggregate(one))
    dropped = ref["dropped"]
    assert dropped.any() and not dropped.all()
    kept_hit = (ref["coverage"] == 1) & ~dropped
    for k, g in enumerate(one):
        np.testing.assert_array_equal(g["coverage"] == 1, kept_hit[k], err_msg=f"{name}: sample {k}")
        assert (g["albedo"][dropped[k]] == 0).all() and (g["normal"][dropped[k]] == 0).all() and np.isposinf(g["depth"][dropped[k]]).all()
        kept = ~dropped[k]
        np.testing.assert_allclose(g["albedo"][kept], ref["albedo"][k][kept], atol=1e-4)
        np.testing.assert_allclose(g["normal"][kept], ref["normal"][k][kept], atol=1e-4)
        np.testing.assert_allclose(g["depth"][kept_hit[k]], ref["depth"][k][kept_hit[k]], rtol=1e-5)
    hits = kept_hit.sum(0)
    # every sample of these pixels hit something, and some were dropped: coverage below 1 because of the drop alone
    partly = dropped.any(0) & (hits > 0) & ((ref["coverage"] == 1).sum(0) == n)
    assert partly.any() and ((0 < hits[partly]) & (hits[partly] < n)).all()
    np.testing.assert_array_equal(window["coverage"], (hits.astype(f32) / f32(n)).astype(f32))
    return int(dropped.sum()), int(partly.sum())


@pytest.mark.parametrize("name", sorted(DROPPED))
def test_dropped_samples_count_in_n_only(name, oracle, emu, built):
    d, desc, cam, p = DROPPED[name]()
    n = p.samples_per_pixel
    one, _ = emu.aov_samples(desc, cam, p, 0, n)
    assert any(g["dropped"].any() for g in one)
    ref = aov_ref.ref_a(oracle, desc, cam, p, list(range(n)))
    for k, g in enumerate(one):
        np.testing.assert_array_equal(g["dropped"], ref["dropped"][k])
    print("\n   dropped samples, pixels partly dropped:", check_dropped_window(name, p, one, emu.aov_window(desc, cam, p, 0, n), ref))
