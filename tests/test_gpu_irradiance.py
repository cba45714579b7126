"""Irradiance queries on the device: vk_trace_irradiance and its per-sample hook.  The hook's directions against the replay of
tests/irradiance_ref.py and its samples against vk_debug_trace_radiance_samples on the replayed rays and resumed streams, on the scenes
of tests/test_rays_emu.py; the public call against the hook by the fixed-point rule (tests/exact_sums.py); point order, batch cuts and
chunks bit for bit; every tree view; no side effect on vk_render; multi-device scenes; degenerate normals.  Every comparison is exact (a
NaN's payload aside) but the last test's, which looks at what the call is for."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_sums
import irradiance_ref as ref
import test_gpu_rays
import test_rays_emu as shared
from vecchio_amd import DeviceScene, ffi
from vecchio_amd.scene import points_from_hits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N, SPP = 193, 4
bits = ref.bits


# ---------------------------------------------------------------- against the radiance query's device path
@pytest.mark.parametrize("kind,name", shared.SCENES, ids=[f"{k}-{n}" for k, n in shared.SCENES])
def test_scene_against_the_radiance_querys_samples(kind, name, device, oracle, host_scenes):
    owner, desc, cam, p = ref.scene(kind, name, host_scenes)
    pts = ref.oracle_points(oracle, desc, cam, p, N)
    ds = DeviceScene(desc)
    try:
        for integ in ref.integrators_allowed(desc, p.integrator):
            kw = ref.params_kwargs(p, seed=p.seed + 17, first_index=2 ** 40 + 5, samples_per_ray=SPP, max_depth=50, integrator=integ)
            samples, dirs, st = ds.debug_irradiance_samples(pts, return_stats=True, **kw)
            assert st.samples == N * SPP and st.kernel_launches == 1 and st.kernel_ms > 0
            rdirs, keys = ref.directions(oracle, pts, **kw)
            ref.assert_same_floats(dirs[..., :3], rdirs, f"{kind} {name} integrator {integ}: directions")
            assert not bits(dirs[..., 3]).any()
            want = ds.debug_radiance_samples(ref.replayed_rays(pts, rdirs), keys.reshape(-1),
                                             **dict(kw, samples_per_ray=1, first_sample=0, first_index=0))
            ref.assert_same_samples(samples, want.reshape(N, SPP, 4), f"{kind} {name} integrator {integ}: samples")
            assert bits(samples[..., 3]).min() >= 2 and bits(samples[..., 3]).max() > 2
    finally:
        ds.close()


# ---------------------------------------------------------------- shared small batches
def probe_rays(cam, n, rng_seed=5):
    """n rays from the camera's origin scattered around its viewing direction"""
    from vecchio_amd.scene import make_rays
    rng = np.random.default_rng(rng_seed)
    o = f32(list(cam.origin))
    look = f32(list(cam.lower_left_corner)) + f32(0.5) * f32(list(cam.horizontal)) + f32(0.5) * f32(list(cam.vertical)) - o
    d = (look + rng.normal(scale=0.3 * float(np.linalg.norm(look)), size=(n, 3))).astype(f32)
    return make_rays(np.tile(o, (n, 1)), d, rng.uniform(float(cam.time0), float(cam.time1), n))


def surface_points(ds, cam, n, rng_seed=5):
    """n points on the scene's surfaces — what the probe rays hit (trace_rays + points_from_hits), repeated up to n — with normals
    that are not unit length and, on every fifth point, a finite tmax"""
    rays = probe_rays(cam, 2 * n, rng_seed)
    pts, index = points_from_hits(ds.trace_rays(rays, 3, 0), rays["time"])
    assert len(pts) > 0 and (pts["time"] == rays["time"][index]).all()
    pts = np.resize(pts, n)
    rng = np.random.default_rng(rng_seed + 1)
    pts["direction"] *= rng.uniform(0.2, 9.0, (n, 1)).astype(f32)
    pts["tmax"][::5] = rng.uniform(0.5, 60.0, len(pts["tmax"][::5])).astype(f32)
    return pts


def kwargs(hs, **over):
    kw = dict(seed=41, first_index=1000, samples_per_ray=1, first_sample=0, max_depth=12, integrator=hs.integrator,
              background=hs.background, background_color=hs.background_color)
    kw.update(over)
    return kw


@pytest.mark.parametrize("name", ["final_scene", "cornell_box", "random_spheres_iow"])
def test_public_call_against_the_hook(name, device, host_scenes):
    """193 points (three full waves of point slots and a partial one) at 1, 37 and 256 samples (256: several sample chunks per block
    of points); a single point at 64 samples; a first_index beyond 2^32"""
    hs, cam = host_scenes(name)
    ds = DeviceScene(hs.desc)
    try:
        all_pts = surface_points(ds, cam, N)
        for n, spp, first_index in ((N, 1, 1000), (N, 37, 1000), (N, 256, 1000), (1, 64, 1000), (N, 8, 2 ** 40)):
            pts = all_pts[:n]
            kw = kwargs(hs, samples_per_ray=spp, first_index=first_index)
            samples, _ = ds.debug_irradiance_samples(pts, **kw)
            want, clamped = exact_sums.exact_image(samples.reshape(-1, 4), n, 1, spp)
            got, st = ds.trace_irradiance(pts, return_stats=True, **kw)
            np.testing.assert_array_equal(bits(got), bits(want.reshape(n, 3)), err_msg=f"{name} n {n} spp {spp}")
            assert st.samples == n * spp and st.kernel_launches == 1 and st.clamped_samples == clamped and st.kernel_ms > 0
            assert np.isfinite(got).all()
            if n > 1:
                assert got.max() > 0
        # the window [3, 8) is rows 3..7 of the window [0, 8); max_depth 0: every sample (0,0,0)
        kw = kwargs(hs, samples_per_ray=8)
        full, fdirs = ds.debug_irradiance_samples(all_pts, **kw)
        win, wdirs = ds.debug_irradiance_samples(all_pts, **dict(kw, samples_per_ray=5, first_sample=3))
        ref.assert_same_samples(win, full[:, 3:8], name)
        ref.assert_same_floats(wdirs, fdirs[:, 3:8], name)
        assert not ds.trace_irradiance(all_pts, **dict(kw, max_depth=0)).any()
        zero, zdirs = ds.debug_irradiance_samples(all_pts, **dict(kw, max_depth=0))
        assert not bits(zero).any() and not bits(zdirs).any()
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["final_scene", "cornell_box", "random_spheres_iow"])
def test_point_order_and_batch_cuts_do_not_show(name, device, host_scenes):
    hs, cam = host_scenes(name)
    ds = DeviceScene(hs.desc)
    try:
        pts = surface_points(ds, cam, N)
        kw = kwargs(hs, samples_per_ray=5)
        samples, dirs = ds.debug_irradiance_samples(pts, **kw)
        whole = ds.trace_irradiance(pts, **kw)
        # 16 points in a permuted order, one call each, each at its own index: the rows of the whole batch
        for j in np.random.default_rng(9).permutation(16):
            one = dict(kw, first_index=kw["first_index"] + int(j))
            s1, d1 = ds.debug_irradiance_samples(pts[j:j + 1], **one)
            ref.assert_same_samples(s1[0], samples[j], f"{name} point {j}")
            ref.assert_same_floats(d1[0], dirs[j], f"{name} point {j}")
            np.testing.assert_array_equal(bits(ds.trace_irradiance(pts[j:j + 1], **one)[0]), bits(whole[j]))
        # the points permuted at one index see other streams (the index, not the point, names the stream)
        assert (bits(ds.debug_irradiance_samples(pts[:16][::-1], **kw)[1][::-1]) != bits(dirs[:16])).any()
        # a batch cut at 100 with first_index continued
        parts = [ds.trace_irradiance(pts[lo:hi], **dict(kw, first_index=kw["first_index"] + lo)) for lo, hi in ((0, 100), (100, N))]
        np.testing.assert_array_equal(bits(np.concatenate(parts)), bits(whole))
    finally:
        ds.close()


def test_the_host_call_works_in_chunks(device, host_scenes):
    """more points than the staging buffer holds (2^20): two launches, and first_index makes the cut invisible"""
    hs, cam = host_scenes("final_scene")
    n = (1 << 20) + 4321
    ds = DeviceScene(hs.desc)
    try:
        pts = np.resize(surface_points(ds, cam, 4096), n)
        kw = kwargs(hs, first_index=2 ** 40, max_depth=4)
        got, st = ds.trace_irradiance(pts, return_stats=True, **kw)
        assert st.kernel_launches == 2 and st.samples == n
        tail = ds.trace_irradiance(pts[-64:], **dict(kw, first_index=2 ** 40 + n - 64))
        np.testing.assert_array_equal(bits(got[-64:]), bits(tail))
        assert (got[:4096] != got[4096:8192]).any()       # the same point at another index draws from another stream
        # the per-sample hook stages 2^22 samples at a time: at 2^21 samples per point three points are two launches (2 + 1), and each
        # point's samples and directions are what a call for that point alone returns
        kw = kwargs(hs, first_index=2 ** 40, max_depth=2, samples_per_ray=1 << 21)
        samples, dirs, st = ds.debug_irradiance_samples(pts[:3], return_stats=True, **kw)
        assert st.kernel_launches == 2 and st.samples == 3 << 21
        for i in range(3):
            s1, d1 = ds.debug_irradiance_samples(pts[i:i + 1], **dict(kw, first_index=2 ** 40 + i))
            np.testing.assert_array_equal(bits(samples[i]), bits(s1[0]), err_msg=f"point {i}")
            np.testing.assert_array_equal(bits(dirs[i]), bits(d1[0]), err_msg=f"point {i}")
    finally:
        ds.close()


# ---------------------------------------------------------------- every view of a scene the walk runs on
_FORM_CHILD = """
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import test_gpu_irradiance as T
from vecchio_amd import DeviceScene, HostScene, ffi
lib = ffi.load_debug_lib() if %(debug)r else None
res = {}
pts = None
for flags in (ffi.VK_SCENE_REFERENCE_TREE, %(flags)d):
    hs = HostScene(%(scene)r, %(seed)d); cam = hs.next_camera()
    hs.desc.contents.flags = flags
    ds = DeviceScene(hs.desc, lib=lib) if lib is not None else DeviceScene(hs.desc)
    if pts is None:
        pts = T.surface_points(ds, cam, 64 * 5 + 3)
    img, st = ds.render(cam, hs.params(64, 2, 50, seed=3))
    res[flags] = (ds.info().tree, bool(st.scene_in_lds), ds.debug_irradiance_samples(pts, **T.kwargs(hs, samples_per_ray=3, max_depth=50)))
    ds.close(); hs.close()
tree, in_lds, (got, gdirs) = res[%(flags)d]
rtree, _, (rgot, rdirs) = res[ffi.VK_SCENE_REFERENCE_TREE]
if %(tree)r is not None:
    assert tree == getattr(ffi, %(tree)r) and in_lds == %(in_lds)r, (tree, in_lds)
assert rtree == ffi.VK_TREE_HANDED_OVER, rtree
assert got[..., 3].view(np.uint32).max() > 2
T.ref.assert_same_floats(gdirs, rdirs, "directions")
T.ref.assert_same_samples(got, rgot, "samples")
print("FORM OK", tree, in_lds)
"""


@pytest.mark.parametrize("form", sorted(test_gpu_rays.FORMS))
def test_every_tree_form_gives_the_reference_trees_samples(form, device):
    scene, seed, env, debug, flags, tree, in_lds = test_gpu_rays.FORMS[form]
    code = _FORM_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), debug=debug, scene=scene, seed=seed, flags=flags, tree=tree,
                              in_lds=in_lds)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FORM OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---------------------------------------------------------------- scene state, devices
def test_an_irradiance_query_leaves_the_render_alone(device, host_scenes):
    for name in ("random_spheres_iow", "cornell_box"):
        hs, cam = host_scenes(name)
        p = hs.params(96, 4, 20, seed=3)
        ds = DeviceScene(hs.desc)
        try:
            pts = surface_points(ds, cam, 200)
            before, _ = ds.render(cam, p)
            ms, requeued = ds.last_kernel_ms(), ds.last_requeued_samples()
            first = ds.trace_irradiance(pts, **kwargs(hs, samples_per_ray=4))
            assert ds.last_kernel_ms() == ms and ds.last_requeued_samples() == requeued
            after, _ = ds.render(cam, p)
            np.testing.assert_array_equal(bits(before), bits(after))
            np.testing.assert_array_equal(bits(ds.trace_irradiance(pts, **kwargs(hs, samples_per_ray=4))), bits(first))
        finally:
            ds.close()


def test_multi_device_scene_answers_from_its_first_device(device, host_scenes):
    hs, cam = host_scenes("final_scene")
    one, multi = DeviceScene(hs.desc), DeviceScene(hs.desc, devices=[0, 0])
    try:
        pts = surface_points(one, cam, 150)
        kw = kwargs(hs, samples_per_ray=4)
        np.testing.assert_array_equal(bits(multi.trace_irradiance(pts, **kw)), bits(one.trace_irradiance(pts, **kw)))
    finally:
        one.close()
        multi.close()


# ---------------------------------------------------------------- degenerate normals
def test_a_zero_normal_sees_the_background_along_a_nan_direction(device, host_scenes):
    """a world of spheres only: 4 points with a zero normal among 60 ordinary ones.  Their axes and direction are NaN, a NaN ray hits no
    sphere: a solid background is returned exactly, the sky's NaN samples are dropped; the other points are untouched by them"""
    hs, cam = host_scenes("random_spheres_iow")
    assert hs.desc.contents.n_rects == 0 and hs.desc.contents.n_media == 0
    ds = DeviceScene(hs.desc)
    try:
        pts = surface_points(ds, cam, 64)
        pts["tmax"] = np.inf
        zero = [3, 17, 40, 63]
        pts["direction"][zero] = 0.0
        bg = (0.25, 0.5, 0.75)
        for background in (ffi.VK_BACKGROUND_SOLID, ffi.VK_BACKGROUND_SKY):
            kw = kwargs(hs, samples_per_ray=4, background=background, background_color=bg)
            got, st = ds.trace_irradiance(pts, return_stats=True, **kw)
            samples, dirs = ds.debug_irradiance_samples(pts, **kw)
            assert np.isnan(dirs[zero][..., :3]).all() and np.isfinite(np.delete(dirs, zero, 0)).all()
            assert (bits(samples[zero][..., 3]) == 2).all()
            if background == ffi.VK_BACKGROUND_SOLID:
                np.testing.assert_array_equal(got[zero], np.tile(f32(bg), (4, 1)))
            else:
                assert np.isnan(samples[zero][..., :3]).any(-1).all()
                assert not bits(got[zero]).any()
            assert np.isfinite(got).all() and st.samples == 64 * 4
            # the ordinary points, asked for without the four in runs that keep their indices
            for lo, hi in ((0, 3), (4, 17), (18, 40), (41, 63)):
                part = ds.trace_irradiance(pts[lo:hi], **dict(kw, first_index=kw["first_index"] + lo))
                np.testing.assert_array_equal(bits(part), bits(got[lo:hi]))
    finally:
        ds.close()


# ---------------------------------------------------------------- what it is for
def test_the_cornell_boxs_floor_is_brightest_below_the_light(device, host_scenes):
    """(sanity, not accuracy) points on the floor from trace_rays + points_from_hits, 64 samples each: every value finite and >= 0, and
    the floor straight below the light (x 213..343, z 227..332 at y = 554) receives more than the floor in the corners"""
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    try:
        rays = ref.pixel_rays(cam, 192, 192)
        pts, index = points_from_hits(ds.trace_rays(rays, 1, 0), 0.0)
        floor = (np.abs(pts["origin"][:, 1]) < 1e-3) & (pts["direction"][:, 1] > 0.99)
        pts = pts[floor]
        x, z = pts["origin"][:, 0], pts["origin"][:, 2]
        below = (x > 213) & (x < 343) & (z > 227) & (z < 332)
        corner = ((x < 70) | (x > 485)) & ((z < 70) | (z > 485))
        assert below.sum() >= 8 and corner.sum() >= 8, (int(below.sum()), int(corner.sum()), len(pts))
        rgb = ds.trace_irradiance(pts, **kwargs(hs, samples_per_ray=64, max_depth=50))
        assert np.isfinite(rgb).all() and (rgb >= 0).all()
        print(f"\n   {len(pts)} floor points: mean below the light {rgb[below].mean():.4f} ({int(below.sum())} points), in the corners "
              f"{rgb[corner].mean():.4f} ({int(corner.sum())} points)")
        assert rgb[below].mean() > rgb[corner].mean()
    finally:
        ds.close()
