"""Occlusion queries on the CPU: vk_trace.h occluded_ray (through tests/emu/emu_occlusion.cpp: the tree view the library promises, the
kernel instance chosen as the launcher chooses it) against the `hit` field of tests/rays_ref.py — one oracle_hit per ray — for exact
equality of every byte, on the scenes and ray sets of tests/test_rays_emu.py.  The output is a bit: no case is left out and there is no
tolerance.  tests/test_gpu_occlusion.py runs the same on the device."""
import numpy as np
import pytest

import rays_ref
import test_rays_emu as shared
from descs import Desc
from vecchio_amd.scene import make_rays

f32 = np.float32


@pytest.fixture(scope="session")
def emu_occ(built):
    import emu_occlusion_ffi
    emu_occlusion_ffi.load()
    return emu_occlusion_ffi


def assert_same_bytes(got, want, what, where=None):
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = np.flatnonzero(got != want.astype(np.uint8))
    if len(bad):
        sets = [k for k, s in (where or {}).items() if s.start <= bad[0] < s.stop]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} bytes differ; first ray {bad[0]} {sets}: got {got[bad[0]]}, want {want[bad[0]]}")


@pytest.mark.parametrize("kind,name", shared.SCENES, ids=[f"{k}-{n}" for k, n in shared.SCENES])
def test_scene_byte_for_byte(kind, name, oracle, emu_occ, host_scenes):
    desc, cam, p = shared.scene(kind, name, host_scenes)
    sets = rays_ref.ray_sets(oracle, desc, cam, p)
    rays, where = rays_ref.all_rays(sets)
    ref = rays_ref.ref_hits(oracle, desc, rays, shared.SEED, 7)["hit"]
    got, features = emu_occ.trace_occluded(desc, rays, shared.SEED, 7)
    print(f"\n   {kind} {name}: features {features:#x}, occluded per set: " +
          ", ".join(f"{k} {int(ref[s].sum())}/{s.stop - s.start}" for k, s in where.items()))
    assert set(np.unique(got)) <= {0, 1}
    assert_same_bytes(got, ref, f"{kind} {name}", where)
    assert ref[where["primary"]].any()
    # a batch cut in two with continuing first_index gives the bytes of the uncut batch
    a = len(rays) // 2 + 1
    parts = [emu_occ.trace_occluded(desc, rays[lo:hi], shared.SEED, 7 + lo)[0] for lo, hi in ((0, a), (a, len(rays)))]
    np.testing.assert_array_equal(np.concatenate(parts), got)


def test_cut_batch_on_a_media_scene_and_the_stream_matters(oracle, emu_occ, host_scenes):
    """final_scene has media: the byte of a ray through fog depends on its stream, i.e. on first_index + i, and on nothing else"""
    desc, cam, p = shared.scene("builder", "final_scene", host_scenes)
    rays, _ = rays_ref.all_rays(rays_ref.ray_sets(oracle, desc, cam, p))
    whole, features = emu_occ.trace_occluded(desc, rays, 77, 2 ** 40)
    assert features != 0
    for cut in (1, 63, len(rays) - 1):
        parts = [emu_occ.trace_occluded(desc, rays[:cut], 77, 2 ** 40)[0], emu_occ.trace_occluded(desc, rays[cut:], 77, 2 ** 40 + cut)[0]]
        np.testing.assert_array_equal(np.concatenate(parts), whole)
    # one ray through a thin fog with nothing behind it within tmax, at 256 indices: both answers occur, each the reference's
    d = Desc()
    from vecchio_amd import ffi
    fog = d.medium(d.sphere((0, 0, -5), 2.0, d.lambertian(0.5, 0.5, 0.5)), 0.2, d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(0.8, 0.8, 0.8)))
    fdesc = d.finish(d.big_box(fog, d.xy_rect(-10, 10, -10, 10, -30.0, d.lambertian(0.1, 0.1, 0.1))))
    same = make_rays([[0, 0, 0]] * 256, [[0, 0, -1]] * 256, tmax=20.0)
    got, _ = emu_occ.trace_occluded(fdesc, same, 5, 1000)
    ref = rays_ref.ref_hits(oracle, fdesc, same, 5, 1000)["hit"]
    assert_same_bytes(got, ref, "thin fog")
    assert 0 < int(got.sum()) < 256


def test_the_interface_rules(oracle, emu_occ):
    """tmax that is a NaN or <= tmin: 0 without a walk; a Rect at exactly tmax counts, a Sphere does not; segment visibility"""
    d, desc = shared._two_objects()          # a unit sphere at z = -5 (t = 4 from the origin), a wall at z = -8
    rays = make_rays([[5, 0, 0]] * 3 + [[0, 0, 0]] * 3, [[0, 0, -1]] * 6,
                     tmax=f32([np.nextafter(f32(8), f32(0)), 8.0, np.nextafter(f32(8), f32(9)), np.nextafter(f32(4), f32(0)), 4.0,
                               np.nextafter(f32(4), f32(5))]))
    got, _ = emu_occ.trace_occluded(desc, rays)
    assert list(got) == [0, 1, 1, 0, 0, 1]
    got, _ = emu_occ.trace_occluded(desc, make_rays([[0, 0, 0]] * 4, [[0, 0, -1]] * 4, tmax=f32([np.nan, 0.001, -1.0, -np.inf])))
    assert list(got) == [0, 0, 0, 0]
    # the segment from a to b is origin a, direction b - a, tmax 1: through the sphere, ending before it, starting behind it
    a = f32([[0, 0, 0], [0, 0, 0], [0, 0, -6.5]])
    b = f32([[0, 0, -7], [0, 0, -3.5], [0, 0, -7.5]])
    seg = make_rays(a, b - a, tmax=1.0)
    got, _ = emu_occ.trace_occluded(desc, seg)
    assert list(got) == [1, 0, 0]
    assert_same_bytes(got, rays_ref.ref_hits(oracle, desc, seg)["hit"], "segments")


def test_fast_accel_view_agrees_with_its_own_closest_hits(emu_occ, oracle, host_scenes):
    """under VK_SCENE_FAST_ACCEL both queries walk the rebuilt tree: the contract is between the two calls on the SAME view"""
    import ctypes as C
    import emu_rays_ffi
    from vecchio_amd import ffi
    hs, cam = host_scenes("random_spheres_iow")
    rays, _ = rays_ref.all_rays(rays_ref.ray_sets(oracle, hs.desc, cam, hs.params(24, 1, 50, seed=7, height=16)))
    fast = ffi.SceneDesc.from_buffer_copy(hs.desc.contents)
    fast.flags |= ffi.VK_SCENE_FAST_ACCEL
    got, _ = emu_occ.trace_occluded(C.pointer(fast), rays, shared.SEED, 0)
    hits, _ = emu_rays_ffi.trace_rays(C.pointer(fast), rays, shared.SEED, 0)
    assert_same_bytes(got, hits["hit"], "fast accel view")
