"""Ray queries on the device: vk_trace_rays and vk_trace_rays_device against tests/rays_ref.py (one oracle_hit per ray) on the scenes and
ray sets of tests/test_rays_emu.py — hit, front, material, object and medium exact for every ray, the float fields within the tolerances
test_aov_emu.check_per_sample applies to the same quantities (normal 1e-4 absolute, t 1e-5 relative, p 1e-5 relative to max(|o|, t |d|),
u and v 1e-4 absolute) — the same hits on every tree form, no side effect on vk_render, multi-device scenes, chunking.  Run with -s for
the number of values that differ bitwise from the oracle and the largest differences."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rays_ref
import test_rays_emu as shared
from vecchio_amd import DeviceScene, HostScene, ffi
from vecchio_amd.scene import HIT_DTYPE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
EXACT = ("hit", "front", "material", "object", "medium")


def check_against_reference(got, ref, rays, what):
    """exact fields for every ray; float fields within the tolerances; returns (bitwise-different float values, worst differences)"""
    for f in EXACT:
        bad = np.flatnonzero(got[f] != ref[f])
        assert len(bad) == 0, f"{what}: {f} differs for {len(bad)} rays; first {bad[0]}: got {got[bad[0]]}, want {ref[bad[0]]}"
    assert (rays_ref.words(got)[:, 14:] == 0).all()
    h = ref["hit"] == 1
    miss = got[~h]
    assert np.isposinf(miss["t"]).all() and not rays_ref.words(miss)[:, [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13]].any(), what
    g, r, q = got[h], ref[h], rays[h]
    # (a NaN ray can "hit" a Rect with a NaN t, and a zero-direction ray one with t = +inf, in the reference as here: a NaN equals a NaN,
    # and equal values — infinities included, whose difference would be a NaN — differ by 0)
    def diff(a, b, scale=None):
        same = (np.isnan(a) & np.isnan(b)) | (a == b)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            if scale is not None:
                d = d / scale
        return np.where(same, 0.0, d)

    worst = {}
    for k in ("normal", "u", "v"):
        d = diff(g[k], r[k])
        assert not np.isnan(d).any() and (d <= 1e-4).all(), f"{what}: {k} off by {np.nanmax(d)}"
        worst[k] = float(d.max()) if d.size else 0.0
    dt = diff(g["t"], r["t"], np.abs(r["t"].astype(np.float64)))
    assert not np.isnan(dt).any() and (dt <= 1e-5).all(), f"{what}: t off by {np.nanmax(dt)} relative"
    with np.errstate(invalid="ignore"):
        scale = np.maximum(np.linalg.norm(q["origin"].astype(np.float64), axis=1),
                           np.abs(r["t"].astype(np.float64)) * np.linalg.norm(q["direction"].astype(np.float64), axis=1))
    dp = diff(g["p"], r["p"], scale[:, None])
    assert not np.isnan(dp).any() and (dp <= 1e-5).all(), f"{what}: p off by {np.nanmax(dp)} relative"
    worst["t_rel"], worst["p_rel"] = float(dt.max()) if dt.size else 0.0, float(dp.max()) if dp.size else 0.0
    gw, rw = rays_ref.words(got)[:, :9], rays_ref.words(ref)[:, :9]
    both_nan = np.isnan(gw.view(f32)) & np.isnan(rw.view(f32))
    return int(((gw != rw) & ~both_nan).sum()), worst


def device_hits(ds, rays, seed, first_index):
    """through vk_trace_rays_device, on torch tensors"""
    import torch
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).to("cuda:0")
    out = ds.trace_rays(d_rays, seed, first_index)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(-1).view(HIT_DTYPE)


@pytest.mark.parametrize("kind,name", shared.SCENES, ids=[f"{k}-{n}" for k, n in shared.SCENES])
def test_scene_against_reference(kind, name, device, oracle, host_scenes):
    desc, cam, p = shared.scene(kind, name, host_scenes)
    rays, where = rays_ref.all_rays(rays_ref.ray_sets(oracle, desc, cam, p))
    ref = rays_ref.ref_hits(oracle, desc, rays, shared.SEED, 7)
    ds = DeviceScene(desc)
    try:
        got, st = ds.trace_rays(rays, shared.SEED, 7, return_stats=True)
        assert st.samples == len(rays) and st.kernel_launches == 1 and st.scene_in_lds == 0 and st.kernel_ms > 0
        n_diff, worst = check_against_reference(got, ref, rays, f"{kind} {name}")
        print(f"\n   {kind} {name}: {len(rays)} rays, {int(ref['hit'].sum())} hits, {int(ref['medium'].sum())} in media; float values that "
              f"differ bitwise from the oracle: {n_diff} of {9 * len(rays)}; worst: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
        # the device-pointer call gives the same bytes
        np.testing.assert_array_equal(rays_ref.words(device_hits(ds, rays, shared.SEED, 7)), rays_ref.words(got))
        # a batch cut in three with matching first_index is the whole batch
        a, b = len(rays) // 3, 2 * len(rays) // 3
        parts = [ds.trace_rays(rays[lo:hi], shared.SEED, 7 + lo) for lo, hi in ((0, a), (a, b), (b, len(rays)))]
        np.testing.assert_array_equal(rays_ref.words(np.concatenate(parts)), rays_ref.words(got))
    finally:
        ds.close()


# ---------------------------------------------------------------- every view of a scene the walk runs on (vk_api.hip aov_view)
# name -> scene, scene seed, environment of the child (read at scene creation), debug library?, flags, tree, staged in LDS?
FORMS = {
    "grid_lds": ("random_spheres_iow", 1, {}, False, 0, "VK_TREE_REBUILT_GRID", True),
    "near_lds": ("random_spheres_iow", 3, {"VK_NO_GRID": "1"}, False, 0, "VK_TREE_REBUILT_NEAR", True),
    "near_global": ("stress_spheres:30", 1, {}, False, 0, "VK_TREE_REBUILT_NEAR", False),        # both trees in one items[]
    "unit_lds": ("random_spheres_iow", 1, {"VK_NEAR_FIRST": "0", "VK_NO_GRID": "1"}, True, 0, "VK_TREE_REBUILT_PROVEN", True),
    "fast_accel": ("random_spheres_iow", 1, {}, False, ffi.VK_SCENE_FAST_ACCEL, None, None),
}

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
    res[flags] = (ds.info().tree, bool(st.scene_in_lds), ds.info().features, ds.trace_rays(rays, 11, 5))
    ds.close(); hs.close()
tree, in_lds, features, got = res[%(flags)d]
rtree, _, rfeatures, rgot = res[ffi.VK_SCENE_REFERENCE_TREE]
if %(tree)r is not None:
    assert tree == getattr(ffi, %(tree)r) and in_lds == %(in_lds)r, (tree, in_lds)
assert rtree == ffi.VK_TREE_HANDED_OVER, rtree
assert features == 0 and rfeatures == 0, (features, rfeatures)
assert got["hit"].sum() > 100
assert np.array_equal(rays_ref.words(got), rays_ref.words(rgot)), np.flatnonzero((rays_ref.words(got) != rays_ref.words(rgot)).any(1))
np.save(%(out)r, got)
print("FORM OK", tree, in_lds)
"""


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_tree_form_gives_the_reference_trees_hits(form, device, oracle, tmp_path):
    """One sphere-only world per view aov_view can return, each in a fresh child process with its own time limit (the switches are read at
    scene creation).  The child asserts the form vk_render runs and that the hits — `object` included — are bit-identical to those of the
    same world created with VK_SCENE_REFERENCE_TREE; the hits then meet the oracle here."""
    scene, seed, env, debug, flags, tree, in_lds = FORMS[form]
    out = str(tmp_path / "hits.npy")
    code = _FORM_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), debug=debug, scene=scene, seed=seed, flags=flags, tree=tree,
                              in_lds=in_lds, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FORM OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(out)
    hs = HostScene(scene, seed)
    cam = hs.next_camera()
    rays, _ = rays_ref.all_rays(rays_ref.ray_sets(oracle, hs.desc, cam, hs.params(24, 1, 50, seed=7, height=16)))
    ref = rays_ref.ref_hits(oracle, hs.desc, rays, 11, 5)
    n_diff, worst = check_against_reference(got, ref, rays, form)
    print(f"\n   {form}: {n_diff} float values differ bitwise from the oracle; worst: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    hs.close()


# ---------------------------------------------------------------- scene state
def test_a_ray_query_leaves_the_render_alone(device, oracle, host_scenes):
    for name in ("random_spheres_iow", "cornell_box"):
        hs, cam = host_scenes(name)
        p = hs.params(96, 4, 20, seed=3)
        rays, _ = rays_ref.all_rays(rays_ref.ray_sets(oracle, hs.desc, cam, hs.params(24, 1, 50, seed=7, height=16)))
        ds = DeviceScene(hs.desc)
        try:
            before, _ = ds.render(cam, p)
            ms = ds.last_kernel_ms()
            requeued = ds.last_requeued_samples()
            first = ds.trace_rays(rays, 3, 0)
            assert ds.last_kernel_ms() == ms and ds.last_requeued_samples() == requeued
            after, _ = ds.render(cam, p)
            np.testing.assert_array_equal(before.view(np.uint32), after.view(np.uint32))
            np.testing.assert_array_equal(rays_ref.words(ds.trace_rays(rays, 3, 0)), rays_ref.words(first))
        finally:
            ds.close()


def test_multi_device_scene_answers_from_its_first_device(device, oracle, host_scenes):
    hs, cam = host_scenes("final_scene")
    rays, _ = rays_ref.all_rays(rays_ref.ray_sets(oracle, hs.desc, cam, hs.params(24, 1, 50, seed=7, height=16)))
    one = DeviceScene(hs.desc)
    multi = DeviceScene(hs.desc, devices=[0, 0])
    try:
        want = one.trace_rays(rays, 9, 100)
        assert want["medium"].any()
        np.testing.assert_array_equal(rays_ref.words(multi.trace_rays(rays, 9, 100)), rays_ref.words(want))
        np.testing.assert_array_equal(rays_ref.words(device_hits(multi, rays, 9, 100)), rays_ref.words(want))
    finally:
        one.close()
        multi.close()


def test_the_host_variant_works_in_chunks(device, oracle, host_scenes):
    """more rays than the staging buffer holds (2^20): the chunks' first_index make the cut invisible, media included"""
    hs, cam = host_scenes("final_scene")
    base, _ = rays_ref.all_rays(rays_ref.ray_sets(oracle, hs.desc, cam, hs.params(24, 1, 50, seed=7, height=16)))
    n = (1 << 20) + 4321
    rays = np.resize(base, n)
    ds = DeviceScene(hs.desc)
    try:
        got, st = ds.trace_rays(rays, 77, 2 ** 40, return_stats=True)
        assert st.kernel_launches == 2 and st.samples == n
        want = device_hits(ds, rays, 77, 2 ** 40)
        np.testing.assert_array_equal(rays_ref.words(got), rays_ref.words(want))
        # the same ray at another index meets another stream: the media hits of the first and second copy of `base` differ somewhere
        k = len(base)
        assert got["medium"][:k].any() and (got["t"][:k] != got["t"][k:2 * k]).any()
        ref = rays_ref.ref_hits(oracle, hs.desc, rays[-64:], 77, 2 ** 40 + n - 64)
        check_against_reference(got[-64:], ref, rays[-64:], "the last rays of the second chunk")
    finally:
        ds.close()


def test_autofocus(device, oracle, host_scenes):
    """what the query is for: the distance under the image centre, through the lens centre"""
    from vecchio_amd.scene import make_rays
    for name in ("cornell_box", "random_spheres_iow"):
        hs, cam = host_scenes(name)
        o = f32(list(cam.origin))
        d = f32(list(cam.lower_left_corner)) + f32(0.5) * f32(list(cam.horizontal)) + f32(0.5) * f32(list(cam.vertical)) - o
        want = oracle.hit(hs.desc, [float(x) for x in o], [float(x) for x in d], float(cam.time0))
        assert want is not None
        ds = DeviceScene(hs.desc)
        try:
            h = ds.trace_rays(make_rays([o], [d], float(cam.time0)))[0]
            assert h["hit"] == 1 and h["material"] == want["material"]
            np.testing.assert_allclose(float(h["t"]) * float(np.linalg.norm(d)), want["t"] * float(np.linalg.norm(d)), rtol=1e-5)
        finally:
            ds.close()
