"""First hits, media, textures and camera rays of the DEVICE against tests/geometry_ref.py (f64 closed forms written from the reference's
lines alone), through public calls: vk_trace_rays on the scenes and rays of tests/test_geometry.py, vk_render_aov on textured carriers,
vk_film_emit + vk_paths_read against the f64 camera, and sphere clouds rendered on every view of a rebuilt tree, where every sample
names the sphere the walk found.  The bounds are geometry_ref.BOUND: four times the ORACLE's deviation from the f64 values, measured on
the CPU; nothing here is derived from what the device returns.  Run with -s for the device's own deviations.

Sizes: a scene's <= 4096 rays in one call, media batches of 20 000 rays, frames of 32 x 24 at <= 4 samples."""
import os
import subprocess
import sys

import numpy as np
import pytest

import geometry_ref as G
import test_geometry as T
from descs import Desc, camera, params
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


# ================================================================ ray queries
@pytest.mark.parametrize("kind,seed", T.SCENES, ids=[f"{k}-{s}" for k, s in T.SCENES])
def test_random_graph(kind, seed, device, oracle):
    g, desc, cam, p, rays, where, sc, want, record = T.scene(kind, seed, oracle)
    ds = DeviceScene(desc)
    try:
        got, st = ds.trace_rays(rays, T.SEED, 7, return_stats=True)
        assert st.samples == len(rays) and st.kernel_launches == 1
        worst = G.compare_hits(got, want, record, rays, f"device {kind} {seed}")
        print(f"\n   {kind} {seed}: {len(rays)} rays, tree {ds.info().tree}; device - f64: " + ", ".join(f"{k} {worst[k]:.3g}" for k in ("t", "p", "normal", "uv")))
        G.assert_within(worst, f"device {kind} {seed}")
    finally:
        ds.close()


def _one(desc, rays, seed=0):
    ds = DeviceScene(desc)
    try:
        return ds.trace_rays(rays, seed, 0)
    finally:
        ds.close()


@pytest.mark.parametrize("name", sorted(T.ROTATIONS))
def test_direct_rotation(name, device):
    d, desc, rays, want = T.rotation_case(name)
    T.check_direct(_one(desc, rays)[0], want, f"device {name}")


@pytest.mark.parametrize("name", ["bare", "translate", "translate_of_flip", "flip_of_translate"])
def test_direct_translate_back_face(name, device):
    d, desc, rays, want = T.translate_cases()[name]
    T.check_direct(_one(desc, rays)[0], want, f"device {name}")


def test_direct_moving_sphere_outside_its_shutter(device):
    d, desc, rays = T.moving_sphere_case()
    T.check_moving_sphere(_one(desc, rays), "device")


def test_direct_rect_bounds_are_inclusive(device):
    d, desc, rays = T.rect_bounds_case()
    T.check_rect_bounds(_one(desc, rays), "device")


def test_checker_at_an_exact_zero_through_a_bounce(device):
    """vk_trace_rays, then one bounce of vk_shade_hits with the scatter integrator: the throughput is the Checker's value at a hit
    point whose z is exactly 0 (test_geometry.checker_zero_case)"""
    from vecchio_amd.scene import make_path_states
    d, desc, rays = T.checker_zero_case()
    ds = DeviceScene(desc)
    try:
        hits = ds.trace_rays(rays, 0, 0)
        shaded = ds.shade_hits(rays, hits, make_path_states(len(rays)), integrator=ffi.VK_INTEGRATOR_SCATTER)
        T.check_checker_zero(hits, shaded, "device")
    finally:
        ds.close()


def test_spherical_uv_over_the_whole_sphere(device):
    d = Desc()
    s = d.sphere((0, 0, 0), 1.0, d.lambertian(0.5, 0.5, 0.5))
    desc = d.finish(d.big_box(s, s))
    rays = T.sphere_uv_rays()
    want, record = G.reference(G.Scene(desc), rays)
    G.assert_within(G.compare_hits(_one(desc, rays), want, record, rays, "device sphere uv"), "device sphere uv")


# ================================================================ media: the ray index is the stream
@pytest.mark.parametrize("name", sorted(T.media_cases()))
def test_medium(name, device):
    d, desc, rays = T.media_rays(name)
    assert len(rays) <= 20000
    z = T.check_medium(desc, rays, _one(desc, rays, T.SEED), f"device {name}")
    print(f"\n   device {name}: z " + ", ".join(f"{k} {v:.2f}" for k, v in z.items()))


# ================================================================ first-hit buffers
def test_first_hit_buffers(device, oracle):
    """vk_render_aov at 1 spp and aperture 0 on Lambertian carriers of image, checker and noise textures: the albedo is the f64 texture
    value at the f64 hit of the pixel's f64 camera ray; normal and depth are that hit's"""
    d, desc = T.carrier_scene()
    c = T.AOV_CAM
    cam = camera(c["lookfrom"], c["lookat"], c["vfov"], c["aspect"], c["aperture"], c["focus"], c["t0"], c["t1"], c["vup"])
    p = params(T.AOV_W, T.AOV_H, 1, seed=T.AOV_SEED, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SOLID)
    want = T.aov_reference(oracle, desc)
    ds = DeviceScene(desc)
    try:
        got, _ = ds.render_aov(cam, p, 0)
        dev = T.check_aov(got, want, "device")
        print(f"\n   first-hit buffers, device - f64: " + ", ".join(f"{k} {v:.3g}" for k, v in dev.items()))
        assert dev["albedo"] <= G.BOUND["aov_albedo"] and dev["normal"] <= G.BOUND["normal"] and dev["t"] <= G.BOUND["t"], dev
    finally:
        ds.close()


# ================================================================ camera
@pytest.fixture(scope="module")
def any_scene(device):
    d = Desc()
    s = d.sphere((0, 0, -100), 1.0, d.lambertian(0.5, 0.5, 0.5))
    ds = DeviceScene(d.finish(d.big_box(s, s)))
    yield ds
    ds.close()


@pytest.mark.parametrize("c", T.CAMERAS, ids=T.camera_id)
def test_camera(c, any_scene, oracle):
    """vk_film_emit + vk_paths_read against the f64 camera: the origin in the lens disc, origin + direction on the focus plane at the
    point of the stream's two draws, the time in [time0, time1), and id ((y - y0) w + (x - x0)) n + k = sample first + k of pixel (x, y) —
    on whole frames and on a window inside the largest one"""
    cam = camera(c["lookfrom"], c["lookat"], c["vfov"], c["aspect"], c["aperture"], c["focus"], c["t0"], c["t1"], c["vup"])
    worst = 0.0
    spp = T.CAM_SPP
    for width, height in T.FRAMES:
        windows = [(0, 0, width, height, 0, spp)] + ([(3, 2, 10, 7, 1, 1)] if (width, height) == (21, 13) else [])
        p = params(width, height, spp, seed=T.CAM_SEED, integrator=ffi.VK_INTEGRATOR_SCATTER)
        xi_all = G.stream_draws(oracle.draws, T.CAM_SEED, width, height, spp)
        with any_scene.film(cam, p) as film, any_scene.paths(width * height * spp) as pb:
            for x0, y0, w, h, first, n in windows:
                film.emit(pb, x0, y0, w, h, first, n)
                ids, rays, states = pb.read()
                assert sorted(ids.tolist()) == list(range(w * h * n))
                order = np.argsort(ids)
                rays, states = rays[order], states[order]
                shape = (h, w, n)
                y, x, k = np.mgrid[y0:y0 + h, x0:x0 + w, first:first + n]
                assert (states["pixel"].reshape(shape) == y * width + x).all() and (states["sample"].reshape(shape) == k).all()
                assert (states["seed"] == T.CAM_SEED).all()
                xi = xi_all[y0:y0 + h, x0:x0 + w, first:first + n]
                worst = max(worst, T.check_camera_rays(c, width, height, rays["origin"].reshape(shape + (3,)),
                                                       rays["direction"].reshape(shape + (3,)), rays["time"].reshape(shape), xi,
                                                       f"device {width}x{height} window {x0},{y0}", x0, y0))
    print(f"\n   {T.camera_id(c)}: device rays - f64 {worst:.3g} of the focus distance")
    assert worst <= G.BOUND["camera"]


# ================================================================ rebuilt trees
# environment of the child (read at scene creation), debug library?
FORMS = {
    "default": ({}, False),
    "no_grid": ({"VK_NO_GRID": "1"}, False),
    "unit": ({"VK_NEAR_FIRST": "0", "VK_NO_GRID": "1"}, True),
}
# what each cloud runs on under each form (vk_scene_get_info().tree): the three small clouds take the near form by default (the grid form
# takes no world of fewer than 72 spheres) and the unit form where VK_NEAR_FIRST=0 asks for it; the 84-sphere layer takes the grid form
# by default and the near form without it, also under VK_NEAR_FIRST=0 (the unit form is not cheap on a layer: its leaf units are long)
N, P, GR = ffi.VK_TREE_REBUILT_NEAR, ffi.VK_TREE_REBUILT_PROVEN, ffi.VK_TREE_REBUILT_GRID
EXPECTED = {(c, "default"): N for c in ("layer", "shared", "inside")}
EXPECTED.update({(c, "no_grid"): N for c in T.CLOUDS})
EXPECTED.update({(c, "unit"): P for c in ("layer", "shared", "inside")})
EXPECTED[("grid", "default")], EXPECTED[("grid", "unit")] = GR, N


def cloud_child(form, out_dir):
    """in the child process: every cloud on the form its environment selects; saves the per-sample dumps and prints what ran"""
    debug = FORMS[form][1]
    lib = ffi.load_debug_lib() if debug else ffi.load_device_lib()
    from test_gpu_parity import device_samples
    for name in T.CLOUDS:
        d, desc, cam, p, scale = T.cloud(name)
        ds = DeviceScene(desc, lib=lib)
        img, ps = device_samples(ds, cam, p)
        launches = ffi.last_launches(lib, ds._h)
        print("CLOUD", name, ds.info().tree, int(any(l.grid_form for l in launches)), int(all(l.lds_scene for l in launches)), len(launches))
        np.save(os.path.join(out_dir, f"{name}.npy"), ps)
        ds.close()
    print("CHILD OK")


@pytest.mark.parametrize("form", sorted(FORMS))
def test_cloud_on_a_rebuilt_tree(form, device, oracle, tmp_path):
    """a fresh child process per environment (the switches are read at scene creation).  Every sample of every cloud names the f64 winner
    of its primary ray.  Which form ran: vk_scene_get_info().tree must be the one EXPECTED names for every cloud; the launch log must
    show grid_form exactly where the tree is the grid's and the scene staged in LDS on every launch (these worlds are small).  The log
    has no field that tells the near form from the unit form: for those two the scene info is the evidence."""
    env, debug = FORMS[form]
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport test_gpu_geometry as M\nM.cloud_child(%r, %r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), form, str(tmp_path)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    ran = {}
    for line in r.stdout.splitlines():
        if line.startswith("CLOUD"):
            _, name, tree, grid, lds, n = line.split()
            ran[name] = (int(tree), int(grid), int(lds), int(n))
    print(f"\n   {form}: " + ", ".join(f"{k} tree {v[0]} grid launch {v[1]} lds {v[2]} launches {v[3]}" for k, v in ran.items()))
    for name in T.CLOUDS:
        tree, grid, lds, n = ran[name]
        assert tree == EXPECTED[(name, form)] and n >= 1, (form, name, ran[name])
        assert grid == (tree == ffi.VK_TREE_REBUILT_GRID) and lds == 1, (form, name, ran[name])
        T.check_cloud(name, np.load(str(tmp_path / f"{name}.npy")), oracle, f"device {name} {form}")


@pytest.mark.parametrize("name", T.CLOUDS)
def test_cloud_on_the_flagged_trees(name, device, oracle):
    from test_gpu_parity import device_samples
    d, desc, cam, p, scale = T.cloud(name)
    for flags, tree in ((ffi.VK_SCENE_REFERENCE_TREE, ffi.VK_TREE_HANDED_OVER), (ffi.VK_SCENE_FAST_ACCEL, ffi.VK_TREE_REBUILT_FAST)):
        desc.contents.flags = flags
        ds = DeviceScene(desc)
        try:
            assert ds.info().tree == tree, (flags, ds.info().tree)
            T.check_cloud(name, device_samples(ds, cam, p)[1], oracle, f"device {name} flags {flags}")
        finally:
            ds.close()
