"""Occlusion queries on the device: vk_trace_occluded and vk_trace_occluded_device against the `hit` field of vk_trace_rays (same process,
same scene, same rays) and of tests/rays_ref.py (one oracle_hit per ray) — exact equality of every byte, as tests/test_gpu_rays.py holds
its `hit` field to the oracle — at the batch lengths around the refill kernel's block of 64 * K rays per wave, on batches that run its
claim loop dry at different moments, through the one-ray-per-lane form of the debug library, across the host variant's chunk boundary, on
every tree form, with no side effect on vk_render, on a multi-device scene."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rays_ref
import test_gpu_rays as R
import test_rays_emu as shared
from descs import Desc
from vecchio_amd import DeviceScene, HostScene, ffi
from vecchio_amd.scene import make_rays

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
K = int(re.search(r"constexpr uint32_t OCC_K = (\d+)u", open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_kernels.h")).read()).group(1))
LENGTHS = (1, 63, 64, 65, 64 * K - 1, 64 * K, 64 * K + 1, 256 * K + 3)
CANARY = 0xAA
SCENES = (("builder", "random_spheres_iow"), ("builder", "cornell_box"), ("builder", "final_scene"))      # spheres only, Cornell, media


def to_device(rays):
    import torch
    return torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda:0")


def device_bytes(ds, rays, seed, first_index, call=None):
    """through vk_trace_occluded_device (or `call`, the debug hook) into the middle of a canary-filled buffer at an odd address: the bytes,
    after checking that nothing around them was written"""
    import torch
    n = len(rays)
    buf = torch.full((n + 129,), CANARY, dtype=torch.uint8, device="cuda:0")
    out = buf[1:1 + n]
    if call is None:
        ds.trace_occluded(to_device(rays), seed, first_index, out=out)
    else:
        call(to_device(rays), out)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[0] == CANARY and (got[1 + n:] == CANARY).all(), "bytes outside occluded[0, n_rays) were written"
    return got[1:1 + n].copy()


def host_bytes(ds, rays, seed, first_index):
    n = len(rays)
    buf = np.full(n + 128, CANARY, np.uint8)
    got, st = ds.trace_occluded(rays, seed, first_index, out=buf[:n], return_stats=True)
    assert st.samples == n and st.kernel_launches == 1 and st.kernel_ms > 0
    assert (buf[n:] == CANARY).all(), "bytes beyond occluded[n_rays - 1] were written"
    return got.copy()


@pytest.fixture(scope="module")
def batches(oracle, host_scenes):
    """per scene: 256 * K + 3 rays (the ray sets of tests/rays_ref.py, repeated) and the oracle's `hit` for one pass over the sets,
    computed once"""
    out = {}
    for kind, name in SCENES:
        desc, cam, p = shared.scene(kind, name, host_scenes)
        base, where = rays_ref.all_rays(rays_ref.ray_sets(oracle, desc, cam, p))
        out[name] = (desc, np.resize(base, LENGTHS[-1]), len(base), where)
    return out


@pytest.mark.parametrize("kind,name", SCENES, ids=[n for _, n in SCENES])
def test_both_entry_points_against_closest_hits_and_the_oracle(kind, name, device, oracle, batches):
    desc, rays, n_base, where = batches[name]
    ds = DeviceScene(desc)
    try:
        want = ds.trace_rays(rays, shared.SEED, 7)["hit"].astype(np.uint8)
        for n in LENGTHS:
            np.testing.assert_array_equal(host_bytes(ds, rays[:n], shared.SEED, 7), want[:n], err_msg=f"{name}: host variant, {n} rays")
            np.testing.assert_array_equal(device_bytes(ds, rays[:n], shared.SEED, 7), want[:n], err_msg=f"{name}: device variant, {n} rays")
        # the oracle: every ray of the sets, exactly (first_index 7, as above)
        ref = rays_ref.ref_hits(oracle, desc, rays[:n_base], shared.SEED, 7)["hit"].astype(np.uint8)
        print(f"\n   {name}: {n_base} rays, {int(ref.sum())} occluded; per set: " +
              ", ".join(f"{k} {int(ref[s].sum())}/{s.stop - s.start}" for k, s in where.items()))
        got = host_bytes(ds, rays[:n_base], shared.SEED, 7)
        bad = np.flatnonzero(got != ref)
        assert len(bad) == 0, f"{name}: {len(bad)} bytes differ from the oracle; first ray {bad[0]}: got {got[bad[0]]}, want {ref[bad[0]]}"
        np.testing.assert_array_equal(device_bytes(ds, rays[:n_base], shared.SEED, 7), ref)
        # a batch cut in two with continuing first_index
        a = n_base // 2 + 1
        parts = [ds.trace_occluded(rays[:a], shared.SEED, 7), ds.trace_occluded(rays[a:n_base], shared.SEED, 7 + a)]
        np.testing.assert_array_equal(np.concatenate(parts), ref)
        assert ds.trace_occluded(rays[:0]).shape == (0,)
    finally:
        ds.close()


def claim_loop_batches(n):
    """on random_spheres_iow (a ground sphere of radius 1000 under y = 0, small spheres up to y = 0.4, three unit spheres on the x axis):
    an immediate hit starts just above the ground and points down; a long miss skims over the small spheres between the large ones"""
    rng = np.random.default_rng(5)
    xz = rng.uniform(-10, 10, (n, 2)).astype(f32)
    hit = make_rays(np.stack([xz[:, 0], np.full(n, 0.01, f32), xz[:, 1]], 1), np.tile(f32([0, -1, 0]), (n, 1)))
    x = (rng.choice(f32([-6, -2, 2, 6]), n) + rng.uniform(-0.1, 0.1, n)).astype(f32)
    miss = make_rays(np.stack([x, np.full(n, 0.45, f32), np.full(n, -15, f32)], 1), np.tile(f32([0, 0, 1]), (n, 1)))
    every = np.arange(n) % 64 == 37
    few_miss, few_hit = hit.copy(), miss.copy()
    few_miss[every], few_hit[every] = miss[every], hit[every]
    return {"all_hit": (hit, np.ones(n, np.uint8)), "all_miss": (miss, np.zeros(n, np.uint8)),
            "a_miss_every_64": (few_miss, (~every).astype(np.uint8)), "a_hit_every_64": (few_hit, every.astype(np.uint8))}


def test_claim_loop_batches_and_the_plain_form(device, host_scenes):
    """the batches on which the refill kernel's waves run dry at different moments; the one-ray-per-lane form of the debug library and
    other (k, t) of the refill form give the same bytes"""
    hs, _ = host_scenes("random_spheres_iow")
    dbg = ffi.load_debug_lib()
    ds, dd = DeviceScene(hs.desc), DeviceScene(hs.desc, lib=dbg)
    tp = ffi.TraceParams(3, 11, 0, 0)

    def hook(refill, k, t):
        def call(d_rays, out):
            st = dbg.vk_debug_trace_occluded_device(dd._h, C.byref(tp), C.c_void_p(d_rays.data_ptr()), d_rays.shape[0],
                                                    C.c_void_p(out.data_ptr()), None, refill, k, t)
            assert st == ffi.VK_OK, dbg.vk_last_error()
        return call

    try:
        for name, (rays, expect) in claim_loop_batches(LENGTHS[-1]).items():
            want = ds.trace_rays(rays, 3, 11)["hit"].astype(np.uint8)
            np.testing.assert_array_equal(want, expect, err_msg=f"{name}: the batch is not what its name says")
            np.testing.assert_array_equal(device_bytes(ds, rays, 3, 11), want, err_msg=name)
            np.testing.assert_array_equal(host_bytes(ds, rays, 3, 11), want, err_msg=name)
            for refill, k, t in ((0, 0, 0), (1, K, 16), (1, 1, 64), (1, 3, 1), (1, 4096, 33)):
                np.testing.assert_array_equal(device_bytes(dd, rays, 3, 11, hook(refill, k, t)), want, err_msg=f"{name} {refill} {k} {t}")
    finally:
        ds.close()
        dd.close()


def test_the_plain_form_on_a_media_scene(device, batches):
    desc, rays, n_base, _ = batches["final_scene"]
    dbg = ffi.load_debug_lib()
    ds, dd = DeviceScene(desc), DeviceScene(desc, lib=dbg)
    tp = ffi.TraceParams(shared.SEED, 7, 0, 0)
    try:
        want = ds.trace_occluded(rays, shared.SEED, 7)
        assert 0 < int(want.sum()) < len(want)
        for refill, k, t in ((0, 0, 0), (1, 2, 8)):
            def call(d_rays, out):
                assert dbg.vk_debug_trace_occluded_device(dd._h, C.byref(tp), C.c_void_p(d_rays.data_ptr()), d_rays.shape[0],
                                                          C.c_void_p(out.data_ptr()), None, refill, k, t) == ffi.VK_OK, dbg.vk_last_error()
            np.testing.assert_array_equal(device_bytes(dd, rays, shared.SEED, 7, call), want)
    finally:
        ds.close()
        dd.close()


def test_the_host_variant_works_in_chunks(device):
    """2^20 + 65 cheap rays on three spheres: two launches, the bytes of the device variant's one launch, the answers known in advance"""
    d = Desc()
    m = d.lambertian(0.5, 0.5, 0.5)
    desc = d.finish(d.big_box(d.sphere((-3, 0, -5), 1.0, m), d.big_box(d.sphere((0, 0, -5), 1.0, m), d.sphere((3, 0, -5), 1.0, m))))
    n = (1 << 20) + 65
    i = np.arange(n)
    x = f32([-3, 0, 3, 1.5])[i % 4]                       # three towards a sphere's centre, one between two spheres
    rays = make_rays(np.stack([x, np.zeros(n, f32), np.zeros(n, f32)], 1), np.tile(f32([0, 0, -1]), (n, 1)),
                     tmax=np.where(i % 8 < 4, np.inf, 3.5).astype(f32))      # every second group of four stops short of the spheres
    expect = ((i % 4 != 3) & (i % 8 < 4)).astype(np.uint8)
    ds = DeviceScene(desc)
    try:
        buf = np.full(n + 64, CANARY, np.uint8)
        got, st = ds.trace_occluded(rays, 1, 2 ** 40, out=buf[:n], return_stats=True)
        assert st.kernel_launches == 2 and st.samples == n and st.kernel_ms > 0
        assert (buf[n:] == CANARY).all()
        np.testing.assert_array_equal(got, expect)
        np.testing.assert_array_equal(device_bytes(ds, rays, 1, 2 ** 40), expect)
    finally:
        ds.close()


_FORM_CHILD = """
import sys, ctypes as C
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import oracle_ffi, rays_ref
from vecchio_amd import DeviceScene, HostScene, ffi
lib = ffi.load_debug_lib() if %(debug)r else None
res = {}
for flags in (%(flags)d, ffi.VK_SCENE_REFERENCE_TREE):
    hs = HostScene(%(scene)r, %(seed)d); cam = hs.next_camera()
    if flags == %(flags)d:
        rays, _ = rays_ref.all_rays(rays_ref.ray_sets(oracle_ffi, hs.desc, cam, hs.params(24, 1, 50, seed=7, height=16)))
    hs.desc.contents.flags = flags
    ds = DeviceScene(hs.desc, lib=lib) if lib is not None else DeviceScene(hs.desc)
    img, st = ds.render(cam, hs.params(128, 8, 50, seed=3))
    res[flags] = (ds.info().tree, bool(st.scene_in_lds), ds.trace_occluded(rays, 11, 5), ds.trace_rays(rays, 11, 5)["hit"])
    ds.close(); hs.close()
tree, in_lds, got, hit = res[%(flags)d]
rtree, _, rgot, rhit = res[ffi.VK_SCENE_REFERENCE_TREE]
if %(tree)r is not None:
    assert tree == getattr(ffi, %(tree)r) and in_lds == %(in_lds)r, (tree, in_lds)
assert rtree == ffi.VK_TREE_HANDED_OVER, rtree
assert got.sum() > 100
assert np.array_equal(got, hit) and np.array_equal(rgot, rhit)
assert np.array_equal(got, rgot), np.flatnonzero(got != rgot)
np.save(%(out)r, got)
print("FORM OK", tree, in_lds)
"""


@pytest.mark.parametrize("form", sorted(R.FORMS))
def test_every_tree_form_gives_the_reference_trees_bytes(form, device, oracle, tmp_path):
    """the forms of tests/test_gpu_rays.py, each in a fresh child process with its own time limit: the bytes equal those of the same world
    created with VK_SCENE_REFERENCE_TREE and the closest-hit query's `hit` on both; here they meet the oracle"""
    scene, seed, env, debug, flags, tree, in_lds = R.FORMS[form]
    out = str(tmp_path / "occluded.npy")
    code = _FORM_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), debug=debug, scene=scene, seed=seed, flags=flags, tree=tree,
                              in_lds=in_lds, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FORM OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(out)
    hs = HostScene(scene, seed)
    cam = hs.next_camera()
    rays, _ = rays_ref.all_rays(rays_ref.ray_sets(oracle, hs.desc, cam, hs.params(24, 1, 50, seed=7, height=16)))
    ref = rays_ref.ref_hits(oracle, hs.desc, rays, 11, 5)["hit"].astype(np.uint8)
    np.testing.assert_array_equal(got, ref)
    hs.close()


def test_an_occlusion_query_leaves_the_render_alone(device, batches, host_scenes):
    for name in ("random_spheres_iow", "cornell_box"):
        hs, cam = host_scenes(name)
        p = hs.params(96, 4, 20, seed=3)
        rays = batches[name][1]
        ds = DeviceScene(hs.desc)
        try:
            before, _ = ds.render(cam, p)
            ms, requeued = ds.last_kernel_ms(), ds.last_requeued_samples()
            first = ds.trace_occluded(rays, 3, 0)
            assert ds.last_kernel_ms() == ms and ds.last_requeued_samples() == requeued
            after, _ = ds.render(cam, p)
            np.testing.assert_array_equal(before.view(np.uint32), after.view(np.uint32))
            np.testing.assert_array_equal(ds.trace_occluded(rays, 3, 0), first)
        finally:
            ds.close()


def test_multi_device_scene_answers_from_its_first_device(device, batches):
    desc, rays, _, _ = batches["final_scene"]
    one = DeviceScene(desc)
    multi = DeviceScene(desc, devices=[0, 0])
    try:
        want = one.trace_occluded(rays, 9, 100)
        assert 0 < int(want.sum()) < len(want)
        np.testing.assert_array_equal(multi.trace_occluded(rays, 9, 100), want)
        np.testing.assert_array_equal(device_bytes(multi, rays, 9, 100), want)
    finally:
        one.close()
        multi.close()
