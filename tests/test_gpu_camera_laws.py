"""The lens, the shutter and what they blur, on the DEVICE, against tests/camera_laws_ref.py (f64 laws written from the reference's lines
alone), through the calls a user makes: vk_film_emit + vk_paths_read and the first read of a regenerating batch for the values and the
laws; vk_render, a vk_progress handle, a film, vk_render_aov's coverage and vk_render_mattes' counts for the frames.  The cases, bounds
and laws are tests/test_camera_laws.py's; nothing here is derived from what the device returns.  Run with -s for the device's figures.

Sizes: frames of at most 33 x 16 at 512 samples (24 x 12 at 2048 for the motion blur); the laws' batch holds 65 536 paths."""
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_laws_ref as L
import geometry_ref as G
import test_camera_laws as T
import test_geometry as TG
from descs import Desc, params
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
FAR = 30.0                       # every camera of parts 1 and 2 sits at the centre of a Lambertian sphere of this radius


# ================================================================ 1. and 2.: emitted rays, and a regenerating batch's first read
@pytest.fixture(scope="module")
def shell_scene(device):
    """a Lambertian sphere of radius FAR round lookfrom = (3, 2, 5): every camera ray meets it and scatters, so a regenerating batch
    holds every path it started after its first bounce"""
    d = Desc()
    s = d.sphere((3, 2, 5), FAR, d.lambertian(0.5, 0.5, 0.5))
    ds = DeviceScene(d.finish(d.big_box(s, s)))
    yield ds
    ds.close()


def read_by_id(pb, n=None):
    ids, rays, states = pb.read()
    if n is not None:
        assert sorted(ids.tolist()) == list(range(n))
    order = np.argsort(ids)
    return ids[order], rays[order], states[order]


def regen_bound(c):
    """A regenerating batch shows a path after its first bounce: the ray starts at the camera ray's hit point p and keeps its time.  The
    lens point is where the line through p and the f64 focus point of the sample's jitter crosses the lens plane.  p deviates by at
    most geometry_ref.BOUND['p'] of its distance FAR, which the line carries to the lens plane over the lever focus / (FAR - focus); the
    focus point of the f32 ray deviates by geometry_ref.BOUND['camera'] of the focus distance.  Relative to the focus distance:"""
    return G.BOUND["p"] * FAR / (FAR - c["focus"]) + G.BOUND["camera"] * FAR / (FAR - c["focus"]) + L.BOUND_LENS


def lens_points_of_hits(c64, st, p):
    """the points of the lens plane (through lookfrom, normal w) on the lines through the hit points p (h, w, n, 3) and the f64 focus
    points of the samples' jitter"""
    x0, y0, w, h = st["window"]
    width, height = st["frame"]
    y, x = np.mgrid[y0:y0 + h, x0:x0 + w]
    F = G.focus_point(c64, *G.pixel_st(st["xi"], x[..., None], y[..., None], width, height))
    dp, dF = (p - c64["origin"]) @ c64["w"], (F - c64["origin"]) @ c64["w"]
    k = dp / (dp - dF)                               # p + k (F - p) has no w component
    return p + k[..., None] * (F - p)


@pytest.mark.parametrize("name,c", T.VALUE_CAMERAS, ids=[n for n, _ in T.VALUE_CAMERAS])
def test_values(name, c, shell_scene, oracle):
    """every sample's lens point and time from its stream's draws: vk_film_emit + vk_paths_read on whole frames and on a window inside
    the larger one, samples from 0 and from 5; and the first read of a regenerating batch on that window, for a capacity below and
    above it"""
    cam, c64 = T.camera_pair(c)
    spp, worst = T.VALUE_SPP, [0.0, 0.0, 0.0]
    for width, height in T.VALUE_FRAMES:
        windows = [(0, 0, width, height)] + ([(3, 2, 10, 7)] if (width, height) == (21, 13) else [])
        for first in T.VALUE_FIRSTS:
            p = params(width, height, first + spp, seed=T.SEED, integrator=ffi.VK_INTEGRATOR_SCATTER)
            with shell_scene.film(cam, p) as film, shell_scene.paths(width * height * spp) as pb:
                for x0, y0, w, h in windows:
                    whole = (x0, y0, w, h) == (0, 0, width, height)
                    st = T.streams(oracle, T.SEED, width, height, first, spp, None if whole else (x0, y0, w, h))
                    shape = (h, w, spp)
                    film.emit(pb, x0, y0, w, h, first, spp)
                    ids, rays, states = read_by_id(pb, w * h * spp)
                    y, x, k = np.mgrid[y0:y0 + h, x0:x0 + w, first:first + spp]
                    assert (states["pixel"].reshape(shape) == y * width + x).all() and (states["sample"].reshape(shape) == k).all()
                    what = f"device {name} {width}x{height} window {x0},{y0} from {first}"
                    lens, dt, _ = T.hold_values(c, c64, st, *T.in_id_order(rays, shape), what)
                    worst = [max(a, b) for a, b in zip(worst, (lens, dt, 0.0))]
                    if whole:
                        continue
                    want_o, _, want_t, unstable = L.get_ray(c64, st)
                    for capacity in (100, w * h * spp + 7):
                        with shell_scene.paths(capacity) as rb:
                            film.regen_begin(rb, x0, y0, w, h, first, spp)
                            info = film.regen_step(rb, 1)
                            n = min(capacity, w * h * spp)
                            assert info.emitted == n and info.live == n, (what, capacity, info.emitted, info.live)
                            ids, rays, states = read_by_id(rb, n)
                        ok = ~unstable.reshape(-1)[:n]
                        dt = np.abs(rays["time"].astype(f64) - want_t.reshape(-1)[:n])[ok].max()
                        assert dt <= L.bound_time(c64["time0"], c64["time1"]), (what, capacity, dt)
                        assert (states["pixel"] == (y * width + x).reshape(-1)[:n]).all() and (states["sample"] == k.reshape(-1)[:n]).all()
                        # (a window's ids run over whole pixels: the first n ids are the first n samples of the arrays, flattened)
                        hit = np.zeros(shape + (3,))
                        hit.reshape(-1, 3)[:n] = rays["origin"].astype(f64)
                        got = lens_points_of_hits(c64, st, hit).reshape(-1, 3)[:n]
                        a, b, _ = G.lens_coordinates(c64, got)
                        wa, wb, _ = G.lens_coordinates(c64, want_o.reshape(-1, 3)[:n])
                        dev = float(np.maximum(np.abs(a - wa), np.abs(b - wb))[ok].max()) / c["focus"]
                        assert dev <= regen_bound(c), (what, capacity, dev, regen_bound(c))
                        worst[2] = max(worst[2], dev)
    print(f"\n   {name}: device - f64: lens {worst[0]:.3g} of the focus distance (bound {L.BOUND_LENS:.3g}), time {worst[1]:.3g}; lens point behind "
          f"a regenerating batch's first bounce {worst[2]:.3g} (bound {regen_bound(c):.3g})")


@pytest.mark.parametrize("name,c", T.LAW_CAMERAS, ids=[n for n, _ in T.LAW_CAMERAS])
def test_laws(name, c, shell_scene, oracle):
    """what the draws add up to, on 64 x 32 x 32 emitted paths and on the same window behind a regenerating batch's first bounce"""
    cam, c64 = T.camera_pair(c)
    W, H = T.LAW_W, T.LAW_H

    def by_emit(seed, spp):
        p = params(W, H, spp, seed=seed, integrator=ffi.VK_INTEGRATOR_SCATTER)
        with shell_scene.film(cam, p) as film, shell_scene.paths(W * H * spp) as pb:
            film.emit(pb, 0, 0, W, H, 0, spp)
            ids, rays, states = read_by_id(pb, W * H * spp)
        o, _, t = T.in_id_order(rays, (H, W, spp))
        return o, t

    def by_regen(seed, spp):
        p = params(W, H, spp, seed=seed, integrator=ffi.VK_INTEGRATOR_SCATTER)
        with shell_scene.film(cam, p) as film, shell_scene.paths(W * H * spp + 7) as rb:
            film.regen_begin(rb, 0, 0, W, H, 0, spp)
            assert film.regen_step(rb, 1).live == W * H * spp
            ids, rays, states = read_by_id(rb, W * H * spp)
        hit, _, t = T.in_id_order(rays, (H, W, spp))
        return lens_points_of_hits(c64, T.streams(oracle, seed, W, H, 0, spp), hit.astype(f64)), t
    for who, route in (("vk_film_emit", by_emit), ("vk_regen_step", by_regen)):
        stats, ctl, failing = T.hold_laws(route, oracle, c, f"device {who} {name}")
        worst = max(stats, key=lambda k: abs(stats[k]["z"]))
        print(f"\n   device {who} {name}: worst |z| {abs(stats[worst]['z']):.2f} ({worst}), repeated {failing}; controls z "
              + ", ".join(f"{k} {z:.1f}" for k, z in ctl.items()))


# ================================================================ 3. frames: the five routes
def matte_count(ids, counts, ref):
    return np.where(ids == ref, counts, 0).sum(-1).astype(np.int64)


def routes(ds, cam, p, emitter, first_window=100, every=True):
    """name -> per-pixel count of the samples that see the emitter, through each call a user can make; at the same seed.  every=False:
    the scene holds other objects, whose hits vk_render_aov's coverage counts too: that route is left out."""
    n = p.samples_per_pixel
    out = {"vk_render": T.counts_of(ds.render(cam, p)[0], n, "vk_render")}
    with ds.progress(cam, p) as pr:
        pr.step(first_window)
        out["vk_progress"] = T.counts_of(pr.step(n - first_window)[0], n, "vk_progress")
    with ds.film(cam, p) as film, ds.paths(1 << 16) as pb:
        for win in film.windows(1 << 16):
            film.emit(pb, *win)
            while pb.step(1).live:
                pass
            film.deposit(pb)
        out["vk_film"] = T.counts_of(film.resolve(), n, "vk_film")
    if every:
        cov = ds.render_aov(cam, p, 0, want=("coverage",))[0]["coverage"].astype(f64) * n
        assert (cov == np.round(cov)).all()
        out["vk_render_aov"] = cov.astype(np.int64)
    ids, counts, over = ds.render_mattes(cam, p, 0)
    assert not over.any()
    out["vk_render_mattes"] = matte_count(ids, counts, emitter)
    return out


def same_counts(r, what):
    first = r["vk_render"]
    for k, v in r.items():
        assert np.array_equal(v, first), f"{what}: {k} counts {int((v != first).sum())} pixels differently from vk_render"
    return first


@pytest.mark.parametrize("name", sorted(T.EDGE_CASES))
def test_defocused_edge(name, device):
    d, desc, cam, c64, p, axis = T.edge_case(name)
    ds = DeviceScene(desc)
    try:
        counts = same_counts(routes(ds, cam, p, ffi.make_ref(ffi.VK_KIND_RECT, 0)), name)
    finally:
        ds.close()
    chi2, m, z, worst = T.hold_edge(name, counts, f"device {name}")
    ctl = T.edge_controls(name, counts)
    print(f"\n   device {name}: five routes agree; {m} partial columns, chi2 {chi2:.1f}, z {z:.2f}, worst column |z| {worst:.2f}; controls z "
          + ", ".join(f"{k} {v:.1f}" for k, v in ctl.items()))
    assert all(v > 8.0 for v in ctl.values()), ctl


NOT_SPHERES = 1 | 2 | 4 | 8 | 16 | 256          # vk_device_scene.h: VKF_MOVING, RECT, LIST, MEDIUM, INSTANCE and BOX, what a scene holds beside spheres


def test_defocused_sphere(device):
    """the sphere-only kernel instance, its scene staged in LDS (the launch log says so), through the lens"""
    d, desc, cam, c64, p = T.sphere_case()
    lib = ffi.load_device_lib()
    ds = DeviceScene(desc)
    try:
        r = routes(ds, cam, p, ffi.make_ref(ffi.VK_KIND_SPHERE, 0), first_window=28, every=False)
        ds.render(cam, p)
        launches = ffi.last_launches(lib, ds._h)
        assert launches and all(l.lds_scene and not (l.features & NOT_SPHERES) for l in launches), [(l.lds_scene, l.features) for l in launches]
    finally:
        ds.close()
    counts = same_counts(r, "sphere")
    chi2, m, z, worst = T.hold_sphere(counts, "device sphere")
    print(f"\n   device sphere: four routes agree; {m} pixels compared, chi2 {chi2:.1f}, z {z:.2f}, worst pixel |z| {worst:.2f}")


def test_motion_blur(device):
    d, desc, cam, c64, p = T.moving_case()
    ds = DeviceScene(desc)
    try:
        counts = same_counts(routes(ds, cam, p, ffi.make_ref(ffi.VK_KIND_MOVING_SPHERE, 0)), "motion blur")
    finally:
        ds.close()
    chi2, m, z, worst = T.hold_cells(counts, T.moving_law(), T.MB_SPP, "device motion blur", 5.0, 60)
    ctl = T.moving_controls(counts)
    print(f"\n   device motion blur: five routes agree; {m} partial pixels, chi2 {chi2:.1f}, z {z:.2f}, worst pixel |z| {worst:.2f}; controls z "
          + ", ".join(f"{k} {v:.1f}" for k, v in ctl.items()))
    assert all(v > 8.0 for v in ctl.values()), ctl


def test_motion_blur_through_a_lens(device):
    d, desc, cam, c64, p = T.moving_case(T.MB_LENS_C, T.MB_LENS_W, T.MB_LENS_H, T.MB_LENS_SPP)
    ds = DeviceScene(desc)
    try:
        counts = same_counts(routes(ds, cam, p, ffi.make_ref(ffi.VK_KIND_MOVING_SPHERE, 0)), "motion blur through a lens")
    finally:
        ds.close()
    chi2, m, z, worst = T.hold_moving_lens(counts, "device motion blur through a lens")
    print(f"\n   device motion blur through a lens: five routes agree; {m} pixels compared, chi2 {chi2:.1f}, z {z:.2f}, worst pixel |z| {worst:.2f}")


# ================================================================ 3. frames: sphere clouds under a lens, on every acceleration form
def cloud_child(form, out_dir):
    """in the child process: every cloud, its camera's aperture opened, on the form the environment selects (test_gpu_geometry.FORMS)"""
    import test_gpu_geometry as GG
    from test_gpu_parity import device_samples
    lib = ffi.load_debug_lib() if GG.FORMS[form][1] else ffi.load_device_lib()
    for name in TG.CLOUDS:
        d, desc, cam, p, scale = T.lens_cloud(name)
        ds = DeviceScene(desc, lib=lib)
        img, ps = device_samples(ds, cam, p)
        launches = ffi.last_launches(lib, ds._h)
        print("CLOUD", name, ds.info().tree, int(any(l.grid_form for l in launches)), int(all(l.lds_scene for l in launches)), len(launches))
        np.save(os.path.join(out_dir, f"{name}.npy"), ps)
        ds.close()
    print("CHILD OK")


@pytest.mark.parametrize("form", ["default", "no_grid", "unit"])
def test_cloud_under_a_lens_on_a_rebuilt_tree(form, device, oracle, tmp_path):
    """test_gpu_geometry.test_cloud_on_a_rebuilt_tree with the lens open: a fresh child per environment; every sample names the f64
    winner of its own f64 ray (part 1's), on the near, unit and grid forms — the one place the megakernel's refill runs a lens on every
    acceleration form"""
    import test_gpu_geometry as GG
    env, debug = GG.FORMS[form]
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport test_gpu_camera_laws as M\nM.cloud_child(%r, %r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), form, str(tmp_path)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    ran = {}
    for line in r.stdout.splitlines():
        if line.startswith("CLOUD"):
            _, name, tree, grid, lds, n = line.split()
            ran[name] = (int(tree), int(grid), int(lds), int(n))
    for name in TG.CLOUDS:
        tree, grid, lds, n = ran[name]
        assert tree == GG.EXPECTED[(name, form)] and n >= 1, (form, name, ran[name])
        assert grid == (tree == ffi.VK_TREE_REBUILT_GRID) and lds == 1, (form, name, ran[name])
        T.check_lens_cloud(name, np.load(str(tmp_path / f"{name}.npy")), oracle, f"device {name} {form}")


@pytest.mark.parametrize("name", TG.CLOUDS)
def test_cloud_under_a_lens_on_the_flagged_trees(name, device, oracle):
    from test_gpu_parity import device_samples
    d, desc, cam, p, scale = T.lens_cloud(name)
    for flags, tree in ((ffi.VK_SCENE_REFERENCE_TREE, ffi.VK_TREE_HANDED_OVER), (ffi.VK_SCENE_FAST_ACCEL, ffi.VK_TREE_REBUILT_FAST)):
        desc.contents.flags = flags
        ds = DeviceScene(desc)
        try:
            assert ds.info().tree == tree, (flags, ds.info().tree)
            T.check_lens_cloud(name, device_samples(ds, cam, p)[1], oracle, f"device {name} flags {flags}")
        finally:
            ds.close()
