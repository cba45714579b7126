"""Radiance queries on the device: vk_trace_radiance and its per-sample hook against the oracle through the bridge of
tests/radiance_ref.py on the scenes of tests/test_rays_emu.py; permutations, windows, chunking and batch cuts bit for bit; the public call
against the hook by the fixed-point rule (tests/exact_sums.py); the first segment against vk_trace_rays; every tree view; no side effect
on vk_render; multi-device scenes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_sums
import radiance_ref
import rays_ref
import test_gpu_rays
import test_rays_emu as shared
from vecchio_amd import DeviceScene, ffi
from vecchio_amd.scene import make_rays

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
W, H, SPP = 20, 12, 4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def integrators_allowed(desc, default):
    """the scene's own integrator first, then the other one where vk_render would take it: the PDF integrator needs lights, the scatter
    integrator a world without SpecDiffuse"""
    d = desc.contents
    ok = {ffi.VK_INTEGRATOR_PDF: d.n_lights > 0,
          ffi.VK_INTEGRATOR_SCATTER: not any(d.materials[i].kind == ffi.VK_MAT_SPEC_DIFFUSE for i in range(d.n_materials))}
    return [default] + [i for i in ok if i != default and ok[i]]


def scene(kind, name, host_scenes):
    """test_rays_emu.scene, which also returns what owns the description's arrays: a radiance sample reads the texels of an image
    texture, which only the Desc that built the scene keeps alive (a ray query never evaluates a material)"""
    import special_scenes
    import test_guides_emu as G
    if kind == "special":
        d, desc, cam, p = special_scenes.ALL[name]()
        return d, desc, cam, p
    if kind == "hand":
        d, desc, cam, p = G.HAND_BUILT[name]()
        return d, desc, cam, p
    return (None,) + tuple(shared.scene(kind, name, host_scenes))


# ---------------------------------------------------------------- the bridge on the device
@pytest.mark.parametrize("kind,name", shared.SCENES, ids=[f"{k}-{n}" for k, n in shared.SCENES])
def test_scene_against_the_oracle(kind, name, device, oracle, host_scenes):
    owner, desc, cam, p0 = scene(kind, name, host_scenes)
    p = ffi.RenderParams.from_buffer_copy(p0)
    p.width, p.height, p.samples_per_pixel, p.max_depth = W, H, SPP, 50
    rays, keys, ref = radiance_ref.bridge(oracle, desc, cam, p)
    ds = DeviceScene(desc)
    try:
        for integ in integrators_allowed(desc, p.integrator):
            if integ != p.integrator:
                p.integrator = integ
                _, ref = oracle.render_samples(desc, cam, p)
            got, st = ds.debug_radiance_samples(rays, keys, return_stats=True, **radiance_ref.radiance_kwargs(p))
            assert st.samples == len(rays) and st.kernel_launches == 1 and st.kernel_ms > 0
            worst = radiance_ref.compare(ref, got)
            print(f"\n   {kind} {name} integrator {integ}: {len(rays)} samples, worst relative radiance error {worst:.3g}")
    finally:
        ds.close()


# ---------------------------------------------------------------- shared small batches
def probe_rays(hs, cam, n, rng_seed=5):
    """n rays from the camera's origin scattered around its viewing direction, some with a finite tmax"""
    rng = np.random.default_rng(rng_seed)
    o = f32(list(cam.origin))
    look = f32(list(cam.lower_left_corner)) + f32(0.5) * f32(list(cam.horizontal)) + f32(0.5) * f32(list(cam.vertical)) - o
    spread = 0.6 * float(np.linalg.norm(look))
    d = (look + rng.normal(scale=spread, size=(n, 3))).astype(f32)
    tmax = np.where(rng.uniform(size=n) < 0.2, rng.uniform(0.5, 3.0, n), np.inf).astype(f32)
    return make_rays(np.tile(o, (n, 1)), d, rng.uniform(float(cam.time0), float(cam.time1), n), tmax)


def kwargs(hs, **over):
    kw = dict(seed=41, first_index=1000, samples_per_ray=1, first_sample=0, max_depth=12, integrator=hs.integrator,
              background=hs.background, background_color=hs.background_color)
    kw.update(over)
    return kw


@pytest.mark.parametrize("name", ["final_scene", "cornell_box", "random_spheres_iow"])
def test_permuting_rays_and_keys_permutes_the_samples(name, device, host_scenes):
    """a single lane, a partial wave, a unit boundary, more waves than one workgroup; sample chunks that do not divide"""
    from vecchio_amd.scene import KEY_DTYPE
    hs, cam = host_scenes(name)
    ds = DeviceScene(hs.desc)
    rng = np.random.default_rng(9)
    try:
        for n in (1, 63, 64, 65, 64 * 17 + 1):
            rays = probe_rays(hs, cam, n)
            keys = np.zeros(n, KEY_DTYPE)
            keys["seed"], keys["pixel"], keys["sample"], keys["ctr"] = 5, rng.integers(0, 1 << 20, n), rng.integers(0, 1000, n), \
                rng.integers(0, 9, n)
            perm = rng.permutation(n)
            for spp in (1, 5, 37):
                kw = kwargs(hs, samples_per_ray=spp)
                a = ds.debug_radiance_samples(rays, keys, **kw)
                b = ds.debug_radiance_samples(rays[perm], keys[perm], **kw)
                assert a.shape == (n, spp, 4)
                np.testing.assert_array_equal(bits(b), bits(a[perm]), err_msg=f"{name} n {n} spp {spp}")
                assert bits(a[..., 3]).max() > 0
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["final_scene", "cornell_box", "random_spheres_iow"])
def test_public_call_against_the_hook(name, device, host_scenes):
    hs, cam = host_scenes(name)
    ds = DeviceScene(hs.desc)
    try:
        n, spp = 64 * 3 + 17, 8
        rays = probe_rays(hs, cam, n)
        kw = kwargs(hs, samples_per_ray=spp)
        samples = ds.debug_radiance_samples(rays, **kw)
        want, clamped = exact_sums.exact_image(samples.reshape(-1, 4), n, 1, spp)
        got, st = ds.trace_radiance(rays, return_stats=True, **kw)
        np.testing.assert_array_equal(bits(got), bits(want.reshape(n, 3)))
        assert st.samples == n * spp and st.kernel_launches == 1 and st.clamped_samples == clamped and st.kernel_ms > 0
        assert np.isfinite(got).all() and got.max() > 0
        # a batch cut in three with continuing first_index gives the same bytes
        a, b = n // 3, 2 * n // 3
        parts = [ds.trace_radiance(rays[lo:hi], **dict(kw, first_index=kw["first_index"] + lo)) for lo, hi in ((0, a), (a, b), (b, n))]
        np.testing.assert_array_equal(bits(np.concatenate(parts)), bits(got))
        # the window [3, 8) is rows 3..7 of the window [0, 8)
        win = ds.debug_radiance_samples(rays, **dict(kw, samples_per_ray=5, first_sample=3))
        np.testing.assert_array_equal(bits(win), bits(samples[:, 3:8]))
        # max_depth 0: every sample (0,0,0)
        assert not ds.trace_radiance(rays, **dict(kw, max_depth=0)).any()
    finally:
        ds.close()


# ---------------------------------------------------------------- the first segment is vk_trace_rays'
@pytest.mark.parametrize("name", ["final_scene", "cornell_box"])
def test_first_segment_is_the_ray_querys(name, device, oracle, host_scenes):
    hs, cam = host_scenes(name)
    rays, where = rays_ref.all_rays(rays_ref.ray_sets(oracle, hs.desc, cam, hs.params(24, 1, 50, seed=7, height=16)))
    bg = (0.25, 0.5, 0.75)
    ds = DeviceScene(hs.desc)
    try:
        hits = ds.trace_rays(rays, 19, 300)
        s = ds.debug_radiance_samples(rays, seed=19, first_index=300, samples_per_ray=1, first_sample=0, max_depth=1,
                                      integrator=hs.integrator, background=ffi.VK_BACKGROUND_SOLID, background_color=bg)[:, 0, :3]
        miss = hits["hit"] == 0
        assert miss.any() and (~miss).any()
        is_bg = (s == f32(bg)).all(1)
        np.testing.assert_array_equal(is_bg, miss)
        odd = where["odd"]
        assert miss[odd][-6:].all()          # a NaN, tiny or negative tmax: a miss without a walk, the path sees the background
        # a hit on something that does not emit: the path ends at max_depth with (0,0,0)
        d = hs.desc.contents
        dark = ~miss & np.array([d.materials[m].kind != ffi.VK_MAT_DIFFUSE_LIGHT for m in hits["material"]])
        assert dark.any()
        finite = np.isfinite(s).all(1)
        assert not s[dark & finite].any()
    finally:
        ds.close()


# ---------------------------------------------------------------- every view of a scene the walk runs on
_FORM_CHILD = """
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import test_gpu_radiance as T
from vecchio_amd import DeviceScene, HostScene, ffi
lib = ffi.load_debug_lib() if %(debug)r else None
res = {}
for flags in (%(flags)d, ffi.VK_SCENE_REFERENCE_TREE):
    hs = HostScene(%(scene)r, %(seed)d); cam = hs.next_camera()
    rays = T.probe_rays(hs, cam, 64 * 5 + 3)
    hs.desc.contents.flags = flags
    ds = DeviceScene(hs.desc, lib=lib) if lib is not None else DeviceScene(hs.desc)
    img, st = ds.render(cam, hs.params(64, 2, 50, seed=3))
    res[flags] = (ds.info().tree, bool(st.scene_in_lds), ds.debug_radiance_samples(rays, **T.kwargs(hs, samples_per_ray=3, max_depth=50)))
    ds.close(); hs.close()
tree, in_lds, got = res[%(flags)d]
rtree, _, rgot = res[ffi.VK_SCENE_REFERENCE_TREE]
if %(tree)r is not None:
    assert tree == getattr(ffi, %(tree)r) and in_lds == %(in_lds)r, (tree, in_lds)
assert rtree == ffi.VK_TREE_HANDED_OVER, rtree
assert got[..., 3].view(np.uint32).max() > 0
assert np.array_equal(got.view(np.uint32), rgot.view(np.uint32)), np.flatnonzero((got.view(np.uint32) != rgot.view(np.uint32)).any((1, 2)))
print("FORM OK", tree, in_lds)
"""


@pytest.mark.parametrize("form", sorted(test_gpu_rays.FORMS))
def test_every_tree_form_gives_the_reference_trees_samples(form, device):
    scene, seed, env, debug, flags, tree, in_lds = test_gpu_rays.FORMS[form]
    code = _FORM_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), debug=debug, scene=scene, seed=seed, flags=flags, tree=tree,
                              in_lds=in_lds)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FORM OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---------------------------------------------------------------- scene state, devices, chunks
def test_a_radiance_query_leaves_the_render_alone(device, host_scenes):
    for name in ("random_spheres_iow", "cornell_box"):
        hs, cam = host_scenes(name)
        p = hs.params(96, 4, 20, seed=3)
        rays = probe_rays(hs, cam, 200)
        ds = DeviceScene(hs.desc)
        try:
            before, _ = ds.render(cam, p)
            ms, requeued = ds.last_kernel_ms(), ds.last_requeued_samples()
            first = ds.trace_radiance(rays, **kwargs(hs, samples_per_ray=4))
            assert ds.last_kernel_ms() == ms and ds.last_requeued_samples() == requeued
            after, _ = ds.render(cam, p)
            np.testing.assert_array_equal(bits(before), bits(after))
            np.testing.assert_array_equal(bits(ds.trace_radiance(rays, **kwargs(hs, samples_per_ray=4))), bits(first))
        finally:
            ds.close()


def test_multi_device_scene_answers_from_its_first_device(device, host_scenes):
    hs, cam = host_scenes("final_scene")
    rays = probe_rays(hs, cam, 150)
    one, multi = DeviceScene(hs.desc), DeviceScene(hs.desc, devices=[0, 0])
    try:
        kw = kwargs(hs, samples_per_ray=4)
        np.testing.assert_array_equal(bits(multi.trace_radiance(rays, **kw)), bits(one.trace_radiance(rays, **kw)))
    finally:
        one.close()
        multi.close()


def test_the_host_call_works_in_chunks(device, host_scenes):
    """more rays than the staging buffer holds (2^20): two launches, and first_index makes the cut invisible"""
    hs, cam = host_scenes("final_scene")
    n = (1 << 20) + 4321
    rays = np.resize(probe_rays(hs, cam, 4096), n)
    ds = DeviceScene(hs.desc)
    try:
        kw = kwargs(hs, first_index=2 ** 40, max_depth=4)
        got, st = ds.trace_radiance(rays, return_stats=True, **kw)
        assert st.kernel_launches == 2 and st.samples == n
        tail = ds.trace_radiance(rays[-64:], **dict(kw, first_index=2 ** 40 + n - 64))
        np.testing.assert_array_equal(bits(got[-64:]), bits(tail))
        assert (got[:4096] != got[4096:8192]).any()       # the same ray at another index draws from another stream
        # the per-sample hook stages 2^22 samples at a time: at 2^21 samples per ray three rays are two launches (2 + 1), and each ray's
        # samples — on its own key's stream, or by the public rule at its own index — are what a call for that ray alone returns
        from vecchio_amd.scene import KEY_DTYPE
        keys = np.zeros(3, KEY_DTYPE)
        keys["seed"], keys["pixel"], keys["sample"], keys["ctr"] = 5, (11, 22, 33), (1, 2, 3), (0, 4, 8)
        kw = kwargs(hs, first_index=2 ** 40, max_depth=2, samples_per_ray=1 << 21)
        for k in (keys, None):
            got, st = ds.debug_radiance_samples(rays[:3], k, return_stats=True, **kw)
            assert st.kernel_launches == 2 and st.samples == 3 << 21
            for i in range(3):
                one = ds.debug_radiance_samples(rays[i:i + 1], None if k is None else k[i:i + 1], **dict(kw, first_index=2 ** 40 + i))
                np.testing.assert_array_equal(bits(got[i]), bits(one[0]), err_msg=f"ray {i}")
    finally:
        ds.close()


# ---------------------------------------------------------------- what it is for
def test_irradiance_probe_in_the_cornell_box(device, host_scenes):
    """64 rays from the room's centre towards a Fibonacci sphere, 64 samples each: the rays that see the light are the bright ones"""
    hs, cam = host_scenes("cornell_box")
    k = np.arange(64) + 0.5
    z = 1.0 - 2.0 * k / 64.0
    phi = np.pi * (1.0 + 5.0 ** 0.5) * k
    r = np.sqrt(1.0 - z * z)
    d = np.stack([r * np.cos(phi), z, r * np.sin(phi)], 1).astype(f32)        # (y up: index 0 looks at the ceiling)
    rays = make_rays(np.tile(f32([278, 278, 278]), (64, 1)), d, 0.0)
    ds = DeviceScene(hs.desc)
    try:
        rgb = ds.trace_radiance(rays, **kwargs(hs, samples_per_ray=64, max_depth=50))
        hits = ds.trace_rays(rays, 41, 1000)
        assert np.isfinite(rgb).all() and (rgb >= 0).all()
        dsc = hs.desc.contents
        on_light = (hits["hit"] == 1) & (hits["front"] == 1) & \
            np.array([dsc.materials[m].kind == ffi.VK_MAT_DIFFUSE_LIGHT for m in hits["material"]])
        assert on_light.any() and (~on_light).any()
        assert rgb[on_light].mean() > rgb[~on_light].mean()
    finally:
        ds.close()
