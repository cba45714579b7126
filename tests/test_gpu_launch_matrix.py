"""-m gpu: every production instance of render_kernel and every launch shape, per sample, with the frame's sums accounted for exactly.

The per-lane arithmetic is covered elsewhere (the emulator, test_gpu_parity.py).  This module reaches the machinery around the lanes:
several units per wave (the straggler branch, the mid-launch flush of the LDS tile sums), uneven and short sample chunks, edge tiles, the
dual launch, scenes in LDS and in global memory, the everything-kernels forced onto sphere-only worlds, the probe (COST) builds and the
dearest-first order, the scheduler thresholds, the forms of exact re-treeing and the redo / fallback launches.

For every run:
  1. the launch log (vk_debug_last_launches) shows the instance and shape the case was written for;
  2. the image is the exact reference of the run's own per-sample dump (tests/exact_sums.py), bit for bit, and so is the clamped count;
  3. the dump (radiance bits and draw counts) and the image are bit-identical to the class's baseline: the default configuration at the
     same size and spp;
  4. once per class, the baseline at the small size passes compare_samples against the oracle.
test_every_instance_was_launched then requires the union of the logged instances to be every render_kernel instance of the product."""
import ctypes as C
import re

import numpy as np
import pytest

import exact_sums
from descs import Desc, camera, params
from test_gpu_parity import compare_samples
from vecchio_amd import DeviceScene, HostScene, build, ffi

pytestmark = pytest.mark.gpu

F_CORNELL = 0x2 | 0x4 | 0x10 | 0x100
F_PDF = 0x80
F_ALL = 0x17F
MAIN, DUAL_1024, DUAL_768, PROBE, REDO, FALLBACK = (ffi.VK_LAUNCH_MAIN, ffi.VK_LAUNCH_DUAL_1024, ffi.VK_LAUNCH_DUAL_768, ffi.VK_LAUNCH_PROBE,
                                                    ffi.VK_LAUNCH_REDO, ffi.VK_LAUNCH_FALLBACK)

LAUNCHED = set()          # (F, LDS_SCENE, MINW, COST, GRID) of every launch logged in this module


# ---- scene classes: one per F that launch_by_features dispatches (and a noise texture among the everything-scenes)
def _bvh(d, items):
    """a median-split BVH over [(ref, lo, hi)] with true bounds"""
    if len(items) == 1:
        return items[0]
    items = sorted(items, key=lambda t: t[1][0] + t[2][0])
    a, b = _bvh(d, items[:len(items) // 2]), _bvh(d, items[len(items) // 2:])
    lo, hi = np.minimum(a[1], b[1]), np.maximum(a[2], b[2])
    return d.bvh_node(a[0], b[0], tuple(lo), tuple(hi)), lo, hi


def sphere_pdf_world():
    """spheres only, an emissive sphere in the lights list: the sphere-only kernel with the PDF integrator"""
    d = Desc()
    rng = np.random.default_rng(7)
    items = []

    def sph(c, r, m):
        c = np.asarray(c, np.float64)
        items.append((d.sphere(tuple(c), r, m), c - abs(r) - 1e-3, c + abs(r) + 1e-3))
        return items[-1][0]

    sph((0, -1000, 0), 1000.0, d.lambertian(0.5, 0.5, 0.5))
    mats = [d.lambertian(0.8, 0.3, 0.2), d.mat(ffi.VK_MAT_METAL, d.solid(0.8, 0.8, 0.7), 0.2), d.mat(ffi.VK_MAT_DIELECTRIC, 0, 1.5),
            d.lambertian(0.2, 0.6, 0.8)]
    for k in range(24):
        c = (rng.uniform(-6, 6), rng.uniform(0.3, 2.0), rng.uniform(-6, 6))
        sph(c, float(rng.uniform(0.3, 0.9)), mats[k % len(mats)])
    lamp = sph((0, 7, 0), 1.5, d.light(8, 8, 8))
    world = _bvh(d, items)[0]
    desc = d.finish(world, lights=[lamp])
    cam = camera((12, 4, 9), (0, 1, 0), vfov=35.0, aspect=1.5)
    return d, desc, cam, ffi.VK_INTEGRATOR_PDF, ffi.VK_BACKGROUND_SOLID, (0.05, 0.05, 0.08)


def _fuzz(pdf):
    from test_fuzz_scenes import Gen
    seed = next(s for s in range(3000, 3100) if bool(np.random.default_rng(s).integers(0, 2)) == pdf)
    g = Gen(seed)
    desc, cam, p = g.build()
    return g, desc, cam, p.integrator, p.background, tuple(p.background_color)


def _builder(name, integrator=None):
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    p = hs.params(16, 1, 50)
    return hs, hs.desc, cam, p.integrator if integrator is None else integrator, p.background, tuple(p.background_color)


CLASSES = {
    # name: (maker, F the frame must launch, max_depth)
    "spheres": (lambda: _builder("random_spheres_iow"), 0, 50),
    "spheres_pdf": (sphere_pdf_world, F_PDF, 50),
    "cornell": (lambda: _builder("cornell_box", ffi.VK_INTEGRATOR_SCATTER), F_CORNELL, 50),
    "cornell_pdf": (lambda: _builder("cornell_box"), F_CORNELL | F_PDF, 50),
    "all": (lambda: _fuzz(False), F_ALL, 16),
    "all_pdf": (lambda: _fuzz(True), F_ALL | F_PDF, 16),
    "noise": (lambda: _builder("perlin_demo"), None, 50),      # (F_ALL with the scene's own integrator: checked in make())
}
_made = {}


def make(cls):
    if cls not in _made:
        maker, F, depth = CLASSES[cls]
        keep, desc, cam, integ, bg_kind, bg = maker()
        if F is None:
            F = F_ALL | (F_PDF if integ == ffi.VK_INTEGRATOR_PDF else 0)
        _made[cls] = (keep, desc, cam, integ, bg_kind, bg, F, depth)
    return _made[cls]


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# sizes (width, height, spp)
SMALL = (67, 45, 8)                 # odd: edge tiles in x and y; one unit per wave or less
SHORT = (67, 45, 37)                # with VK_CHUNK_CAP=8: five chunks of 7, 7, 8, 7, 8 samples
MEDIUM = (128, 96, 64)              # 192 tiles: the probe launch runs (>= 64 tiles, >= 64 spp); 64 tiles per rank of three


def dual_size():
    """>= CUs x 112 units per 24-sample window at one sample per unit (VK_CHUNK_CAP=1): the dual launch's threshold (vk_api.hip)"""
    tiles = -(-cus() * 112 // 24)
    rows = -(-tiles // 40)
    return (320, 8 * rows, 48)


def render(cls, env, size, monkeypatch, tile_world=1, progressive=None):
    """one frame of class `cls` under the switches `env`: (image, dump, launch log, scene info, clamped samples).  The switches are read
    when the scene is created.  tile_world > 1: the frame as tile_world partitions (one scene, one dump and log per rank, merged)."""
    keep, desc, cam, integ, bg_kind, bg, F, depth = make(cls)
    w, h, spp = size
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, str(v))
        ds = DeviceScene(desc)
    lib = ds._lib
    lib.vk_debug_render_samples.restype = C.c_int
    lib.vk_debug_render_samples.argtypes = [C.c_void_p, C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_void_p, C.c_void_p]
    try:
        info = ds.info()
        img = np.zeros((h, w, 3), np.float32)
        dump = np.zeros((w * h * spp, 4), np.float32)
        logs, clamped = [], 0
        tile_of = (np.arange(h)[:, None] // 8) * ((w + 7) // 8) + (np.arange(w)[None, :] // 8)
        for rank in range(tile_world):
            p = params(w, h, spp, max_depth=depth, seed=5, integrator=integ, background=bg_kind, bg=bg, tile_rank=rank, tile_world=tile_world)
            if progressive:
                with ds.progress(cam, p) as pr:
                    for n in progressive:
                        out, _ = pr.step(n)
                img[:] = out
                logs.append(ffi.last_launches(lib, ds._h))
                continue
            mine = np.zeros((w * h * spp, 4), np.float32)
            st = lib.vk_debug_render_samples(ds._h, C.byref(cam), C.byref(p), img.ctypes.data, mine.ctypes.data)
            assert st == 0, lib.vk_last_error().decode()
            c = C.c_uint64()
            assert lib.vk_scene_last_clamped_samples(ds._h, C.byref(c)) == 0
            clamped += c.value
            logs.append(ffi.last_launches(lib, ds._h))
            sel = np.repeat((tile_of % tile_world == rank).reshape(-1), spp)
            dump[sel] = mine[sel]
        for log in logs:
            for r in log:
                LAUNCHED.add((r.features, bool(r.lds_scene), r.minw, bool(r.cost), bool(r.grid_form)))
        return img, dump, logs, info, clamped
    finally:
        ds.close()


_baselines = {}


def baseline(cls, size, monkeypatch, oracle=None):
    """the default configuration at this size (assertion 3's reference); at SMALL also checked against the oracle (assertion 4)"""
    key = (cls, size)
    if key not in _baselines:
        img, dump, logs, info, clamped = render(cls, {}, size, monkeypatch)
        check_exact(img, dump, clamped, size)
        check_log(cls, logs[0], info, "default", size)
        if size == SMALL and oracle is not None:
            keep, desc, cam, integ, bg_kind, bg, F, depth = make(cls)
            w, h, spp = size
            p = params(w, h, spp, max_depth=depth, seed=5, integrator=integ, background=bg_kind, bg=bg)
            img_o, ps_o = oracle.render_samples(desc, cam, p)
            compare_samples(ps_o, dump, img_o, img)
        _baselines[key] = (img, dump)
    return _baselines[key]


def check_exact(img, dump, clamped, size):
    """assertion 2: the image is the exact fixed-point reference of the run's own samples, bit for bit; so is the clamped count"""
    w, h, spp = size
    want, n_clamped = exact_sums.exact_image(dump, w, h, spp)
    bad = want.view(np.uint32) != img.view(np.uint32)
    assert not bad.any(), f"{int(bad.any(axis=2).sum())} pixels differ from the sums of their own samples, first at {np.argwhere(bad)[0]}"
    assert clamped == n_clamped


def check_same(a, b, what):
    da, db = a.view(np.uint32), b.view(np.uint32)
    diff = (da != db).any(axis=-1)
    assert not diff.any(), f"{what}: {int(diff.sum())} differ, first at index {np.argwhere(diff)[0]}"


# ---- configurations: (switches, size, what the launch log must show)
def mains(log):
    return [r for r in log if r.role == MAIN]


def check_log(cls, log, info, case, size):
    """assertion 1: the instance and shape this case was written for"""
    F = make(cls)[6]
    roles = [r.role for r in log]
    frame = [r for r in log if r.role in (MAIN, DUAL_1024, DUAL_768)]
    assert frame, (case, roles)
    w, h, spp = size
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    sphere_only = (F & ~F_PDF) == 0
    forced = case == "force_full"
    want_F = (F_ALL | (F & F_PDF)) if forced else F
    assert all(r.features == want_F for r in log), (case, [(r.role, r.features) for r in log])
    assert info.features == (F_ALL if forced else F & ~F_PDF), (case, info.features)
    if case == "many_units":
        r = mains(log)[0]
        waves = r.grid_size * r.block_size // 64
        assert tiles * spp >= 4 * waves, (case, tiles * spp, waves)          # VK_CHUNK_CAP=1: a unit per tile and sample
    if case in ("dual", "dual_progressive", "dual_retree0"):
        assert DUAL_1024 in roles and DUAL_768 in roles and MAIN not in roles, (case, roles)
        assert all(r.grid_size == cus() for r in frame), (case, [r.grid_size for r in frame])
    else:
        assert DUAL_1024 not in roles and DUAL_768 not in roles, (case, roles)
    if case in ("no_lds", "tile_order_no_lds", "grid_global", "tile_order_grid_global"):
        assert not any(r.lds_scene for r in log), (case, [(r.role, r.lds_scene) for r in log])
    if case.startswith("tile_order"):
        probes = [r for r in log if r.role == PROBE]
        assert len(probes) == 1 and probes[0].cost and not any(r.cost for r in frame), (case, roles)
    else:
        assert PROBE not in roles, (case, roles)
    if forced:
        assert info.tree in (ffi.VK_TREE_HANDED_OVER, ffi.VK_TREE_REBUILT_FAST) and REDO not in roles
        assert not any(r.grid_form for r in log)
    if cls == "spheres":
        grid = [r.grid_form for r in frame]
        if case in ("default", "many_units", "short_chunk", "defer_1", "defer_64", "tile_order", "tile_order_world3", "dual",
                    "dual_progressive", "progressive", "redo_cap", "no_dual"):
            assert info.tree == ffi.VK_TREE_REBUILT_GRID and all(grid), (case, info.tree, grid)
        if case in ("grid_global", "tile_order_grid_global"):
            assert info.tree == ffi.VK_TREE_REBUILT_GRID and all(grid), (case, info.tree, grid)
        if case in ("no_grid", "tile_order_no_grid", "no_lds", "tile_order_no_lds"):
            assert info.tree in (ffi.VK_TREE_REBUILT_NEAR, ffi.VK_TREE_REBUILT_PROVEN) and not any(grid), (case, info.tree, grid)
        if case in ("retree0", "dual_retree0"):
            assert info.tree == ffi.VK_TREE_HANDED_OVER and REDO not in roles and not any(grid), (case, info.tree, roles)
        if info.tree == ffi.VK_TREE_REBUILT_GRID:
            # the grid form (staged in LDS or not): every frame has the second launch and the fallback behind it, on the tree as handed over
            assert roles.count(REDO) == 1 and roles.count(FALLBACK) == 1, (case, roles)
            assert all(r.lds_scene == frame[0].lds_scene and not r.grid_form and not r.cost for r in log if r.role in (REDO, FALLBACK))
    elif sphere_only and not forced:
        assert not any(r.grid_form for r in log)


COMMON = [
    # (case, switches, size)
    ("default", {}, SMALL),
    ("no_lds", {"VK_NO_LDS_SCENE": 1}, SMALL),
    ("force_full", {"VK_FORCE_FULL_VARIANT": 1}, SMALL),
    ("defer_1", {"VK_SHADE_DEFER": 1, "VK_PRIM_WEIGHT": 1}, SMALL),
    ("defer_64", {"VK_SHADE_DEFER": 64, "VK_PRIM_WEIGHT": 64}, SMALL),
    ("short_chunk", {"VK_CHUNK_CAP": 8}, SHORT),
    ("many_units", {"VK_CHUNK_CAP": 1, "VK_MAX_WAVES_PER_CU": 4}, MEDIUM),
    ("progressive", {"VK_CHUNK_CAP": 1, "VK_MAX_WAVES_PER_CU": 4}, MEDIUM),
    ("tile_order", {"VK_TILE_ORDER": 1}, MEDIUM),
    ("tile_order_world3", {"VK_TILE_ORDER": 1}, MEDIUM),
    ("tile_order_no_lds", {"VK_TILE_ORDER": 1, "VK_NO_LDS_SCENE": 1}, MEDIUM),
]
SPHERE_ONLY = [
    ("dual", {"VK_CHUNK_CAP": 1}, "dual"),
    ("dual_progressive", {"VK_CHUNK_CAP": 1}, "dual"),
    ("no_dual", {"VK_CHUNK_CAP": 1, "VK_NO_DUAL_LAUNCH": 1}, "dual"),
]
GRID_FORMS = [       # the forms of exact re-treeing on the scatter scene (the grid form is its default)
    ("grid_global", {"VK_NO_LDS_SCENE": 1, "VK_GRID_GLOBAL": 1}, SMALL),
    ("tile_order_grid_global", {"VK_TILE_ORDER": 1, "VK_NO_LDS_SCENE": 1, "VK_GRID_GLOBAL": 1}, MEDIUM),
    ("no_grid", {"VK_NO_GRID": 1}, SMALL),
    ("tile_order_no_grid", {"VK_TILE_ORDER": 1, "VK_NO_GRID": 1}, MEDIUM),
    ("retree0", {"VK_RETREE": 0}, SMALL),
    ("dual_retree0", {"VK_CHUNK_CAP": 1, "VK_RETREE": 0}, "dual"),
    ("redo_cap", {"VK_REDO_REGION_CAP": 1}, SMALL),
]
CASES = [(cls, *c) for cls in CLASSES for c in COMMON]
CASES += [(cls, *c) for cls in ("spheres", "spheres_pdf") for c in SPHERE_ONLY]
CASES += [("spheres", *c) for c in GRID_FORMS]


@pytest.mark.parametrize("cls,case,env,size", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_launch_shape_per_sample(cls, case, env, size, device, oracle, monkeypatch):
    if size == "dual":
        size = dual_size()
    base_img, base_dump = baseline(cls, size, monkeypatch, oracle)
    baseline(cls, SMALL, monkeypatch, oracle)                # (assertion 4, once per class)
    progressive = None
    if case == "progressive":
        progressive = (5, 11, 48)                          # windows of 5 / 11 / 48 samples: 80 / 176 / 768 units per tile row of 16
    if case == "dual_progressive":
        progressive = (24, 24)                             # each window alone reaches the dual launch's threshold
    img, dump, logs, info, clamped = render(cls, env, size, monkeypatch, tile_world=3 if case == "tile_order_world3" else 1,
                                            progressive=progressive)
    for log in logs:
        check_log(cls, log, info, case, size)
    if progressive:
        # the frame accumulated over the windows is the one-shot frame of the same switches, bit for bit
        one, one_dump, one_logs, _, one_clamped = render(cls, env, size, monkeypatch)
        check_exact(one, one_dump, one_clamped, size)
        check_same(img, one, "progressive frame against the one-shot frame")
        img, dump = one, one_dump
    else:
        check_exact(img, dump, clamped, size)
    check_same(dump.reshape(-1, 4), base_dump.reshape(-1, 4), f"{case}: samples against the default configuration's")
    check_same(img, base_img, f"{case}: pixels against the default configuration's")


def test_forced_everything_kernel_on_a_rebuilt_world_renders_the_handed_over_tree(device, monkeypatch):
    """VK_FORCE_FULL_VARIANT=1 on a world of spheres with exact re-treeing: the everything-kernel cannot walk a rebuilt tree (nor the grid
    form), so the scene is uploaded with the tree as handed over (vk_api.hip create_on_device) and every launch of it gets that view"""
    keep, desc, cam, integ, bg_kind, bg, F, depth = make("spheres")
    with monkeypatch.context() as m:
        ds0 = DeviceScene(desc)
        m.setenv("VK_FORCE_FULL_VARIANT", "1")
        ds1 = DeviceScene(desc)
    try:
        assert ds0.info().tree == ffi.VK_TREE_REBUILT_GRID
        inf = ds1.info()
        assert inf.features == F_ALL and inf.tree == ffi.VK_TREE_HANDED_OVER
    finally:
        ds0.close(); ds1.close()


# ---- coverage: every render_kernel instance of the product was launched above
NEVER_LAUNCHED = {
    # (F, LDS_SCENE, MINW, COST, GRID): the vk_api.hip line that shows why the product cannot launch it.  (Empty: every instance runs.)
}


def product_instances():
    txt = open(build.kernel_resources_path()).read()
    out = set()
    for m in re.finditer(r"render_kernelILj(\d+)ELb([01])ELi(\d+)ELb([01])ELb([01])ELb([01])E", txt):
        assert m.group(4) == "0", "the product library holds no STATS build"
        out.add((int(m.group(1)), m.group(2) == "1", int(m.group(3)), m.group(5) == "1", m.group(6) == "1"))
    return out


def test_every_instance_was_launched(device):
    """runs after the cases above (module order): a render_kernel instance that no case launched fails here, so a new instance needs a
    case (or an entry in NEVER_LAUNCHED with the reason)"""
    assert LAUNCHED, "run with the whole module: the cases above fill the launch set"
    have = product_instances()
    assert LAUNCHED <= have, sorted(LAUNCHED - have)
    missing = have - LAUNCHED - set(NEVER_LAUNCHED)
    assert not missing, sorted(missing)
