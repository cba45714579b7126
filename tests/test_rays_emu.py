"""Ray queries on the CPU: vk_trace.h trace_ray (through tests/emu/emu_rays.cpp, on the tree view the library promises, the kernel instance
chosen as the launcher chooses it, the lineariser's provenance tables) against tests/rays_ref.py — one oracle_hit per ray on a description
whose records each own their material — bit for bit on every field of every ray (a NaN's payload aside).  Also the reference's own
self-tests against closed forms.  tests/test_gpu_rays.py runs the same scenes and ray sets on the device."""
import numpy as np
import pytest

import rays_ref
import special_scenes
import test_guides_emu as G
from descs import Desc
from vecchio_amd import ffi
from vecchio_amd.scene import make_rays

f32 = np.float32


@pytest.fixture(scope="session")
def emu_rays(built):
    import emu_rays_ffi
    emu_rays_ffi.load()
    return emu_rays_ffi


# ---------------------------------------------------------------- scenes (shared with tests/test_gpu_rays.py)
def scene(kind, name, host_scenes):
    """(desc, cam, p) of a builder scene, a hand-built scene of test_guides_emu, a special scene or a fuzz graph"""
    if kind == "builder":
        return G.builder(host_scenes, name)
    if kind == "hand":
        return G.HAND_BUILT[name]()[1:]
    if kind == "special":
        d, desc, cam, p = special_scenes.ALL[name]()
        p.width, p.height = G.W, G.H
        return desc, cam, p
    return G.fuzz(name)


SCENES = [("builder", n) for n in G.BUILDERS] + [("hand", n) for n in sorted(G.HAND_BUILT)] + \
    [("special", n) for n in sorted(special_scenes.ALL)] + [("fuzz", s) for s in G.FUZZ_SEEDS]
SEED = 0xC0FFEE12345


def describe(hits, where):
    return ", ".join(f"{k} {int(hits['hit'][s].sum())}/{s.stop - s.start}" for k, s in where.items())


# ---------------------------------------------------------------- self-tests of the reference against closed forms
def _two_objects():
    d = Desc()
    sph = d.sphere((0, 0, -5), 1.0, d.lambertian(0.5, 0.5, 0.5))
    wall = d.xy_rect(-10, 10, -10, 10, -8.0, d.lambertian(0.5, 0.5, 0.5))      # the same material index as a different record
    return d, d.finish(d.big_box(sph, wall))


def test_ref_sphere_at_a_known_t(oracle):
    d, desc = _two_objects()
    rays = make_rays([[0, 0, 0], [0, 0, 0], [5, 0, 0]], [[0, 0, -1], [0, 0, -2], [0, 0, -1]])
    h = rays_ref.ref_hits(oracle, desc, rays)
    assert list(h["hit"]) == [1, 1, 1]
    np.testing.assert_array_equal(h["t"], f32([4.0, 2.0, 8.0]))           # t is in units of |d|
    np.testing.assert_array_equal(h["p"], f32([[0, 0, -4], [0, 0, -4], [5, 0, -8]]))
    np.testing.assert_array_equal(h["normal"], f32([[0, 0, 1], [0, 0, 1], [0, 0, 1]]))
    assert list(h["front"]) == [1, 1, 1] and list(h["medium"]) == [0, 0, 0]
    assert list(h["object"]) == [ffi.make_ref(ffi.VK_KIND_SPHERE, 0)] * 2 + [ffi.make_ref(ffi.VK_KIND_RECT, 0)]
    # the material is the description's own index, not the duplicate's
    assert list(h["material"]) == [d.spheres[0].material, d.spheres[0].material, d.rects[0].material]
    np.testing.assert_allclose(h["u"][2], 0.75, atol=1e-6)
    np.testing.assert_allclose(h["v"][2], 0.5, atol=1e-6)


def test_ref_rect_at_exactly_tmax_is_accepted_and_a_sphere_is_not(oracle):
    d, desc = _two_objects()
    rays = make_rays([[5, 0, 0]] * 3 + [[0, 0, 0]] * 3, [[0, 0, -1]] * 6,
                     tmax=f32([np.nextafter(f32(8), f32(0)), 8.0, np.nextafter(f32(8), f32(9)), np.nextafter(f32(4), f32(0)), 4.0,
                               np.nextafter(f32(4), f32(5))]))
    h = rays_ref.ref_hits(oracle, desc, rays)
    assert list(h["hit"]) == [0, 1, 1, 0, 0, 1]
    # behind the sphere at exactly tmax = 4 nothing else lies within tmax: a miss is all zeros and t = +inf
    assert np.isposinf(h["t"][4]) and not rays_ref.words(h[4:5])[0, [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]].any()
    # the interface's own rule: a NaN tmax, tmax <= tmin
    h = rays_ref.ref_hits(oracle, desc, make_rays([[0, 0, 0]] * 3, [[0, 0, -1]] * 3, tmax=f32([np.nan, 0.001, -1.0])))
    assert not h["hit"].any()


def test_ref_seed_rule_wraps(oracle):
    assert rays_ref.ray_seed(0, 1) == rays_ref.GOLDEN
    assert rays_ref.ray_seed(2 ** 64 - 1, 1) == rays_ref.GOLDEN - 1
    assert rays_ref.ray_seed(5, 2 ** 32) == (5 + (rays_ref.GOLDEN << 32)) % 2 ** 64
    # a medium's draw is the stream of ray first_index + i: the same ray at another index scatters elsewhere, at the same index the same
    d = Desc()
    fog = d.medium(d.sphere((0, 0, -5), 2.0, d.lambertian(0.5, 0.5, 0.5)), 0.4, d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(0.8, 0.8, 0.8)))
    desc = d.finish(d.big_box(fog, d.xy_rect(-10, 10, -10, 10, -9.0, d.lambertian(0.1, 0.1, 0.1))))
    rays = make_rays([[0, 0, 0]] * 8, [[0, 0, -1]] * 8)
    a = rays_ref.ref_hits(oracle, desc, rays, seed=2 ** 64 - 3, first_index=0)
    b = rays_ref.ref_hits(oracle, desc, rays[3:], seed=2 ** 64 - 3, first_index=3)
    rays_ref.assert_bit_identical(a[3:], b)
    assert len(set(a["t"].tolist())) > 1 and (a["medium"] == 1).any() and (a["medium"] == 0).any()
    m = a[a["medium"] == 1][0]
    assert m["object"] == ffi.make_ref(ffi.VK_KIND_MEDIUM, 0) and m["material"] == d.media[0].material and m["front"] == 1
    assert 3.0 < m["t"] < 7.0 and list(m["normal"]) == [1, 0, 0]


# ---------------------------------------------------------------- the emulator against the reference
@pytest.mark.parametrize("kind,name", SCENES, ids=[f"{k}-{n}" for k, n in SCENES])
def test_scene_bit_for_bit(kind, name, oracle, emu_rays, host_scenes):
    desc, cam, p = scene(kind, name, host_scenes)
    rays, where = rays_ref.all_rays(rays_ref.ray_sets(oracle, desc, cam, p))
    ref = rays_ref.ref_hits(oracle, desc, rays, SEED, 7)
    got, features = emu_rays.trace_rays(desc, rays, SEED, 7)
    print(f"\n   {kind} {name}: features {features:#x}, hits per set: {describe(ref, where)}; media hits {int(ref['medium'].sum())}")
    for k, s in where.items():
        rays_ref.assert_bit_identical(got[s], ref[s], f"{kind} {name}, set {k}")
    assert ref["hit"][where["primary"]].any()
    # a batch cut in three with matching first_index is the whole batch
    a, b = len(rays) // 3, 2 * len(rays) // 3
    parts = [emu_rays.trace_rays(desc, rays[lo:hi], SEED, 7 + lo)[0] for lo, hi in ((0, a), (a, b), (b, len(rays)))]
    np.testing.assert_array_equal(rays_ref.words(np.concatenate(parts)), rays_ref.words(got))


def test_every_kind_of_object_is_named(oracle, emu_rays, host_scenes):
    """over the scenes above: spheres, moving spheres, rects (bare, in lists, as Boxy faces, under instances) and media all win somewhere"""
    kinds = set()
    for kind, name in (("builder", "final_scene"), ("builder", "cornell_box"), ("special", "nested_transforms"), ("hand", "glass_and_media")):
        desc, cam, p = scene(kind, name, host_scenes)
        rays, _ = rays_ref.all_rays(rays_ref.ray_sets(oracle, desc, cam, p))
        got, _ = emu_rays.trace_rays(desc, rays, SEED, 0)
        kinds |= set((got["object"][got["hit"] == 1] >> 28).tolist())
        d = desc.contents
        for k, n in ((ffi.VK_KIND_SPHERE, d.n_spheres), (ffi.VK_KIND_MOVING_SPHERE, d.n_moving_spheres), (ffi.VK_KIND_RECT, d.n_rects),
                     (ffi.VK_KIND_MEDIUM, d.n_media)):
            sel = (got["hit"] == 1) & ((got["object"] >> 28) == k)
            assert ((got["object"][sel] & 0x07FFFFFF) < max(n, 1)).all()
    assert kinds == {ffi.VK_KIND_SPHERE, ffi.VK_KIND_MOVING_SPHERE, ffi.VK_KIND_RECT, ffi.VK_KIND_MEDIUM}, kinds


def test_fast_accel_view_names_the_same_objects(oracle, emu_rays, host_scenes):
    """VK_SCENE_FAST_ACCEL walks the rebuilt tree: re-treeing reorders the visits, not the provenance"""
    hs, cam = host_scenes("random_spheres_iow")
    p = hs.params(G.W, 1, 50, seed=7, height=G.H)
    rays, _ = rays_ref.all_rays(rays_ref.ray_sets(oracle, hs.desc, cam, p))
    plain, _ = emu_rays.trace_rays(hs.desc, rays, SEED, 0)
    fast = ffi.SceneDesc.from_buffer_copy(hs.desc.contents)
    fast.flags |= ffi.VK_SCENE_FAST_ACCEL
    import ctypes as C
    got, _ = emu_rays.trace_rays(C.pointer(fast), rays, SEED, 0)
    same = rays_ref.words(got) == rays_ref.words(plain)
    # (results may differ where a hit lies a rounding error outside its box: include/vecchio_amd.h on VK_SCENE_FAST_ACCEL)
    assert same.all(1).mean() > 0.99
    np.testing.assert_array_equal(got["object"][same.all(1)], plain["object"][same.all(1)])
