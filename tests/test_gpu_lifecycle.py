"""-m gpu: what a handle owns goes with it.  The debug library counts the live device buffers, pinned buffers, events and streams of
its handles (vk_debug_live_objects, vecchio_amd/csrc/vk_resources.h); every test here reads the counts first (other fixtures may hold
scenes of the debug library), uses entry points that allocate lazily, destroys the handles and wants the counts back where they were.

The sphere world is a 9 x 9 layer of small spheres on a ground sphere: the lineariser's grid form wants 72 spheres or more, 64 of them
in the layer (vk_linearize.cpp rt_build_grid), so 9 x 9 is the smallest square layer that takes it — a 6 x 6 layer is walked in the near
form, without the grid's table and second launch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from descs import Desc, camera, params
from vecchio_amd import DeviceScene, HostScene, ffi
from vecchio_amd.scene import make_rays

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
BUFFERS, PINNED, EVENTS, STREAMS = range(4)


def live(lib):
    out = (C.c_uint64 * 4)()
    assert lib.vk_debug_live_objects(C.byref(out)) == ffi.VK_OK, lib.vk_last_error().decode()
    return tuple(out)


def layer_world():
    """(keep-alive, desc, camera, params maker) of the sphere layer: no lights, so the scatter integrator under the sky"""
    d = Desc()
    rng = np.random.default_rng(11)
    items = []

    def sph(c, r, m):
        c = np.asarray(c, np.float64)
        items.append((d.sphere(tuple(c), r, m), c - abs(r) - 1e-3, c + abs(r) + 1e-3))

    def bvh(it):
        if len(it) == 1:
            return it[0]
        it = sorted(it, key=lambda t: t[1][0] + t[2][0])
        a, b = bvh(it[:len(it) // 2]), bvh(it[len(it) // 2:])
        lo, hi = np.minimum(a[1], b[1]), np.maximum(a[2], b[2])
        return d.bvh_node(a[0], b[0], tuple(lo), tuple(hi)), lo, hi

    sph((0, -1000, 0), 1000.0, d.lambertian(0.5, 0.5, 0.5))
    mats = [d.lambertian(0.8, 0.3, 0.2), d.mat(ffi.VK_MAT_METAL, d.solid(0.8, 0.8, 0.7), 0.2), d.mat(ffi.VK_MAT_DIELECTRIC, 0, 1.5)]
    n = 9
    for a in range(n):
        for b in range(n):
            sph((a - n / 2 + 0.9 * rng.uniform(), 0.2, b - n / 2 + 0.9 * rng.uniform()), 0.2, mats[(a * n + b) % 3])
    desc = d.finish(bvh(items)[0])
    cam = camera((9, 2.5, 6), (0, 0.2, 0), vfov=30.0, aspect=1.0)

    def mk(w, h, spp, depth=8, **kw):
        return params(w, h, spp, max_depth=depth, seed=5, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SKY, **kw)

    return d, desc, cam, mk


def cornell_world():
    hs = HostScene("cornell_box", 1)
    cam = hs.next_camera()

    def mk(w, h, spp, depth=8, **kw):
        return hs.params(w, spp, depth, height=h, **kw)      # (the scene's own integrator: PDF)

    return hs, hs.desc, cam, mk


WORLDS = {"layer": layer_world, "cornell": cornell_world}


def every_entry_point(kind, lib):
    """Creates the scene of WORLDS[kind] on `lib` (the debug library), calls every entry-point family on it and destroys it:
    (counts before, counts with the scene and a progress handle alive, counts after, vk_scene_info)."""
    keep, desc, cam, mk = WORLDS[kind]()
    lib.vk_debug_render_samples.restype = C.c_int
    lib.vk_debug_render_samples.argtypes = [C.c_void_p, C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_void_p, C.c_void_p]
    base = live(lib)
    ds = DeviceScene(desc, lib=lib)
    info = ds.info()
    p = mk(32, 32, 8)
    color, _ = ds.render(cam, p)
    p8 = mk(32, 32, 8)
    p8.output_format = ffi.VK_OUTPUT_RGB8
    ds.render(cam, p8)
    img, dump = np.zeros((32, 32, 3), np.float32), np.zeros((32 * 32 * 8, 4), np.float32)
    assert lib.vk_debug_render_samples(ds._h, C.byref(cam), C.byref(p), img.ctypes.data, dump.ctypes.data) == ffi.VK_OK, lib.vk_last_error()
    assert np.array_equal(img, color)
    # 64 local tiles at 64 spp: the smallest shape that reaches the tile-order probe
    ds.render(cam, mk(128, 64, 64, tile_rank=1, tile_world=2))
    assert any(r.role == ffi.VK_LAUNCH_PROBE for r in ffi.last_launches(lib, ds._h))
    ds.render_aov(cam, mk(16, 16, 8))
    aov, _ = ds.render_aov(cam, p)                       # (the staging buffer regrows)
    ds.render_guides(cam, p)
    rng = np.random.default_rng(3)
    hits = ds.trace_rays(make_rays(np.tile(np.float32(cam.origin[:]), (100, 1)), rng.normal(size=(100, 3))))
    assert hits.shape == (100,)
    ds.denoise(color, albedo=aov["albedo"], normal=aov["normal"], depth=aov["depth"])
    with ds.temporal(32, 32) as t:
        t.accumulate(cam, color, aov["normal"], aov["depth"])
        t.accumulate(cam, color, aov["normal"], aov["depth"], want_history=True)
    pr = ds.progress(cam, mk(32, 32, 16), adaptive=dict(abs_tol=1e-3, rel_tol=0.0))      # (implies VK_PROGRESS_STDERR)
    for _ in range(3):
        pr.step(4)
    assert pr.stderr().shape == (32, 32, 3)
    mid = live(lib)
    pr.close()
    ds.close()
    return base, mid, live(lib), info


def check_counts(base, mid, end):
    assert mid[BUFFERS] > base[BUFFERS] and mid[EVENTS] > base[EVENTS], (base, mid)      # the counter is wired to the real owners
    assert end == base, (base, mid, end)


def in_child(code, env):
    """Runs `code` in a fresh interpreter (the library reads its switches once per process); its last line of output."""
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (ROOT, TESTS) + code
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().splitlines()[-1]


@pytest.mark.parametrize("kind", ["layer", "layer_no_lds", "cornell"])
def test_every_entry_point_then_destroy(kind, device):
    """(a) the sphere layer staged in LDS: the grid form, exact re-treeing's queues and verdict slots, the dual launch's stream and
    events; (b) the same world under VK_NO_LDS_SCENE=1 (a child process): both trees in one array, no second launch; (c) the Cornell
    box with the PDF integrator.  After vk_render (f32, RGB8, the per-sample dump, a partition that probes its tile order), the first-hit
    buffers at two sizes, the guides, a ray query, the denoiser, a temporal and an adaptive progressive handle: nothing is left."""
    if kind == "layer_no_lds":
        line = in_child("import test_gpu_lifecycle as T; from vecchio_amd import ffi\n"
                        "base, mid, end, info = T.every_entry_point('layer', ffi.load_debug_lib())\n"
                        "print(repr((base, mid, end, info.lds_bytes, info.tree)))\n", {"VK_NO_LDS_SCENE": "1"})
        base, mid, end, lds_bytes, tree = eval(line)
        assert lds_bytes == 0 and tree != ffi.VK_TREE_REBUILT_GRID, (lds_bytes, tree)
        check_counts(base, mid, end)
        return
    base, mid, end, info = every_entry_point(kind, ffi.load_debug_lib())
    if kind == "layer":
        assert info.tree == ffi.VK_TREE_REBUILT_GRID and info.lds_bytes != 0, (info.tree, info.lds_bytes)
        assert mid[STREAMS] > base[STREAMS] and mid[PINNED] > base[PINNED], (base, mid)      # the dual launch's stream, the verdict slots
    check_counts(base, mid, end)


def group_lifecycle(lib):
    """a group over devices [0, 0, 0]: (counts before, with the group and a progress handle alive, after, the gather it uses)"""
    hs = HostScene("cornell_box", 1)
    cam = hs.next_camera()
    hs.desc.contents.flags |= ffi.VK_SCENE_RCCL_GATHER
    base = live(lib)
    m = DeviceScene(hs.desc, devices=[0, 0, 0], lib=lib)
    gather = m.info().gather
    m.render(cam, hs.params(64, 8, 8, height=48, output_format=ffi.VK_OUTPUT_RGB8))
    pr = m.progress(cam, hs.params(64, 8, 8, height=48))
    pr.step(4)
    pr.step(4)
    m.render_aov(cam, hs.params(32, 4, 8, height=32))
    mid = live(lib)
    pr.close()
    m.close()
    return base, mid, live(lib), gather


def test_group_lifecycle(device):
    """A multi-device group (the device listed three times, slabs through the RCCL test double as tests/test_gpu_abi2.py runs it): the
    parts' streams, slabs and landing buffers — which live on devices[0], not on the part's device — the receive stream and the
    per-part running sums of a progressive handle all go with their handles."""
    from vecchio_amd import build
    mock = build.build_mock_rccl()
    line = in_child("import test_gpu_lifecycle as T; from vecchio_amd import ffi\n"
                    "print(repr(T.group_lifecycle(ffi.load_debug_lib())))\n", {"VK_RCCL_LIB": mock, "VK_RCCL_ALLOW_DUPLICATE_DEVICES": "1"})
    base, mid, end, gather = eval(line)
    assert gather == ffi.VK_GATHER_RCCL, gather
    assert mid[STREAMS] >= base[STREAMS] + 4, (base, mid)      # three parts' streams and the receive stream
    check_counts(base, mid, end)


def test_failed_group_creation_leaves_nothing(device, host_scenes):
    lib = ffi.load_debug_lib()
    hs, _ = host_scenes("cornell_box")
    base = live(lib)
    h = C.c_void_p()
    assert lib.vk_scene_create_multi(hs.desc, (C.c_int * 2)(0, 9999), 2, C.byref(h)) == ffi.VK_ERR_BAD_ARG and not h.value
    assert live(lib) == base


def test_regrow_does_not_accumulate(device, host_scenes):
    """the first-hit buffers' staging buffer grows in place: alternating sizes leave ONE buffer behind, however many calls"""
    lib = ffi.load_debug_lib()
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc, lib=lib)
    counts = []
    for k in range(10):
        side = 16 if k % 2 == 0 else 32
        ds.render_aov(cam, hs.params(side, 4, 8, height=side))
        counts.append(live(lib)[BUFFERS])
    ds.close()
    assert counts[1] == counts[9], counts
