"""First-hit buffers (vk_render_aov) on the MI355X: per sample against the two oracle references of tests/aov_ref.py — media scenes
included, every sample compared: a medium's distance comes from the radiance sample's own stream (oracle_first_hits) — on every view of a
scene the first-hit walk runs on (each form of exact re-treeing bit for bit against the tree as handed over, in a child process per
form; VK_SCENE_FAST_ACCEL), both kernel instances, the same first hit as the radiance sample, medium statistics, exact aggregation with
dropped samples, every call shape bit for bit, non-interference with vk_render and progress handles, invalid calls.  tests/test_aov_emu.py
is the CPU counterpart and holds the shared scenes.  Run with -s for the largest differences per channel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aov_ref
import special_scenes
import test_aov_emu as shared
from descs import Desc, camera, params
from test_fuzz_scenes import Gen
from vecchio_amd import DeviceScene, HostScene, ffi

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = ("cornell_box", "random_spheres_iow", "bowser_demo", "perlin_demo", "balls_demo")


def named(name, width=24, spp=1):
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    p = hs.params(width, spp, 50, seed=7, height=width)
    return hs, hs.desc, cam, p


def fuzz(seed):
    g = Gen(1000 + seed)
    desc, cam, p = g.build()
    return g, desc, cam, p


def singles(ds, cam, p, samples):
    """one call per sample (first_sample = s, spp = 1)"""
    q = ffi.RenderParams()
    C.pointer(q)[0] = p
    q.samples_per_pixel = 1
    return [ds.render_aov(cam, q, first_sample=s)[0] for s in samples]


def _check_against_a(ds, desc, cam, p, oracle, samples=(0, 1)):
    got = singles(ds, cam, p, samples)
    ref = aov_ref.ref_a(oracle, desc, cam, p, list(samples))
    assert np.isfinite(ref["albedo"]).all() and not ref["dropped"].any()         # no sample is left out of a comparison
    worst = shared.Worst()
    for k, g in enumerate(got):
        worst.add(g, ref, k)
    print("\n   device vs oracle:", worst)
    for k, g in enumerate(got):
        med = ref["medium"][k]
        assert (g["normal"][med] == 0).all() and (g["coverage"][med] == 1).all()
        np.testing.assert_array_equal(g["coverage"], ref["coverage"][k])
        hit = ref["coverage"][k] == 1
        np.testing.assert_allclose(g["normal"], ref["normal"][k], atol=1e-4)
        np.testing.assert_allclose(g["depth"][hit], ref["depth"][k][hit], rtol=1e-5)
        assert np.isinf(g["depth"][~hit]).all()
        known = np.isfinite(ref["albedo"][k]).all(-1)
        np.testing.assert_allclose(g["albedo"][known], ref["albedo"][k][known], atol=1e-4)
    return got


def _check_against_b(ds, desc, cam, p, oracle, n=2):
    q = ffi.RenderParams()
    C.pointer(q)[0] = p
    q.samples_per_pixel = n
    ref = aov_ref.ref_b_albedo(oracle, desc, cam, q)
    got = singles(ds, cam, p, range(n))
    for s in range(n):
        np.testing.assert_allclose(got[s]["albedo"], ref[s], atol=1e-4)


@pytest.mark.parametrize("name", NAMED)
def test_named_scene_per_sample_against_oracle(name, device, oracle):
    hs, desc, cam, p = named(name)
    ds = DeviceScene(desc)
    try:
        _check_against_a(ds, desc, cam, p, oracle)
        _check_against_b(ds, desc, cam, p, oracle)
    finally:
        ds.close()


@pytest.mark.parametrize("seed", shared.FUZZ_SEEDS)      # tests/test_fuzz_scenes.py Gen(1000 + seed), with and without media
def test_fuzz_graph_per_sample_against_oracle(seed, device, oracle):
    g, desc, cam, p = fuzz(seed)
    ds = DeviceScene(desc)
    try:
        _check_against_a(ds, desc, cam, p, oracle)
    finally:
        ds.close()


def _media_scene(name):
    if name in NAMED_MEDIA:
        return named(name, width=16)
    if name in shared.EXTRA:
        return shared.EXTRA[name]()
    return shared.special(name)


NAMED_MEDIA = ("final_scene", "final_scene_nextweek")


@pytest.mark.parametrize("name", NAMED_MEDIA + ("media_and_textures", "fog", "camera_inside_medium"))
def test_media_scene_per_sample_against_oracle(name, device, oracle):
    """several media along a ray, a medium under a transform, a Boxy boundary, the camera inside a medium, the single-object BVH node
    that draws its medium twice: normal, depth, coverage and albedo of every sample"""
    keep, desc, cam, p = _media_scene(name)
    ds = DeviceScene(desc)
    try:
        _check_against_a(ds, desc, cam, p, oracle, samples=(0, 1, 2, 3))
        ref = aov_ref.ref_a(oracle, desc, cam, p, [0, 1, 2, 3])
        shared.assert_both_kinds_of_hit(ref)
    finally:
        ds.close()


@pytest.mark.parametrize("name", sorted(special_scenes.ALL))
def test_special_scene_per_sample_against_oracle(name, device, oracle):
    keep, desc, cam, p = shared.special(name)
    ds = DeviceScene(desc)
    try:
        _check_against_a(ds, desc, cam, p, oracle)
    finally:
        ds.close()


# ---------------------------------------------------------------- every view of a scene the first-hit walk runs on (vk_api.hip aov_view)
# name -> scene, scene seed, environment of the child (the switches are read at scene creation), debug library?, tree, staged in LDS?
FORMS = {
    "grid_lds": ("random_spheres_iow", 1, {}, False, "VK_TREE_REBUILT_GRID", True),
    "near_lds": ("random_spheres_iow", 3, {"VK_NO_GRID": "1"}, False, "VK_TREE_REBUILT_NEAR", True),
    "near_global": ("stress_spheres:30", 1, {}, False, "VK_TREE_REBUILT_NEAR", False),        # both trees in one items[]
    "unit_lds": ("random_spheres_iow", 1, {"VK_NEAR_FIRST": "0", "VK_NO_GRID": "1"}, True, "VK_TREE_REBUILT_PROVEN", True),
}
FORM_W, FORM_SAMPLES = 48, (0, 1)

_FORM_CHILD = """
import sys, ctypes as C
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
from vecchio_amd import DeviceScene, HostScene, ffi
lib = ffi.load_debug_lib() if %(debug)r else None
res = {}
for flags in (0, ffi.VK_SCENE_REFERENCE_TREE):
    hs = HostScene(%(scene)r, %(seed)d); hs.desc.contents.flags = flags; cam = hs.next_camera()
    ds = DeviceScene(hs.desc, lib=lib) if lib is not None else DeviceScene(hs.desc)
    img, st = ds.render(cam, hs.params(128, 8, 50, seed=3))
    tree, in_lds, features = ds.info().tree, bool(st.scene_in_lds), ds.info().features
    got = []
    for s in %(samples)r:
        got.append(ds.render_aov(cam, hs.params(%(w)d, 1, 50, seed=7, height=%(w)d), first_sample=s)[0])
    again, _ = ds.render(cam, hs.params(128, 8, 50, seed=3))
    assert np.array_equal(img.view(np.uint32), again.view(np.uint32))
    res[flags] = (tree, in_lds, features, got)
    ds.close(); hs.close()
tree, in_lds, features, got = res[0]
rtree, _, rfeatures, rgot = res[ffi.VK_SCENE_REFERENCE_TREE]
assert tree == ffi.%(tree)s and in_lds == %(in_lds)r, (tree, in_lds)
assert rtree == ffi.VK_TREE_HANDED_OVER, rtree
assert features == 0 and rfeatures == 0, (features, rfeatures)
for a, b in zip(got, rgot):
    for ch in ("albedo", "normal", "depth", "coverage"):
        assert np.array_equal(a[ch].view(np.uint32), b[ch].view(np.uint32)), ch
np.savez(%(out)r, **{"%%s_%%d" %% (ch, k): g[ch] for k, g in enumerate(got) for ch in g})
print("FORM OK", tree, in_lds)
"""


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_tree_view_gives_the_handed_over_trees_first_hits(form, device, oracle, tmp_path):
    """One sphere-only world per form of exact re-treeing, each in a fresh child process (the switches are read at scene creation).  The
    child asserts the form it runs (vk_scene_info.tree, vk_stats.scene_in_lds of a vk_render) and that the per-sample buffers are those
    of the same world created with VK_SCENE_REFERENCE_TREE, bit for bit; the buffers then meet reference (a) here."""
    scene, seed, env, debug, tree, in_lds = FORMS[form]
    out = str(tmp_path / "aov.npz")
    code = _FORM_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), debug=debug, scene=scene, seed=seed, samples=FORM_SAMPLES,
                              w=FORM_W, tree=tree, in_lds=in_lds, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FORM OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    hs = HostScene(scene, seed)
    cam = hs.next_camera()
    p = hs.params(FORM_W, 1, 50, seed=7, height=FORM_W)
    ref = aov_ref.ref_a(oracle, hs.desc, cam, p, list(FORM_SAMPLES))
    assert np.isfinite(ref["albedo"]).all() and not ref["dropped"].any() and 0 < ref["coverage"].sum()
    worst = shared.Worst()
    for k in range(len(FORM_SAMPLES)):
        g = {ch: z["%s_%d" % (ch, k)] for ch in aov_ref.CHANNELS}
        np.testing.assert_array_equal(g["coverage"], ref["coverage"][k])
        hit = ref["coverage"][k] == 1
        np.testing.assert_allclose(g["normal"], ref["normal"][k], atol=1e-4)
        np.testing.assert_allclose(g["depth"][hit], ref["depth"][k][hit], rtol=1e-5)
        assert np.isinf(g["depth"][~hit]).all()
        np.testing.assert_allclose(g["albedo"], ref["albedo"][k], atol=1e-4)
        worst.add(g, ref, k)
    print("\n   %s, device vs oracle:" % form, worst)
    hs.close()


def _fast_accel_scenes():
    from test_retree import Crowd
    out = {"crowd%d" % k: (lambda k=k: (None,) + Crowd(5000 + k).build()) for k in range(4)}

    def iow():
        hs = HostScene("random_spheres_iow", 1)
        hs.desc.contents.flags = ffi.VK_SCENE_FAST_ACCEL
        return hs, hs.desc, hs.next_camera(), hs.params(24, 1, 50, seed=7, height=24)
    out["random_spheres_iow"] = iow
    return out


@pytest.mark.parametrize("name", ["crowd0", "crowd1", "crowd2", "crowd3", "random_spheres_iow"])
def test_fast_accel_first_hits_against_oracle(name, device, oracle):
    """VK_SCENE_FAST_ACCEL: the walk runs on the rebuilt tree with its tie table.  The scenes are those on which the suite requires the
    radiance under this flag to be the reference's (tests/test_retree.py: the crowds, the InOneWeekend world)."""
    keep, desc, cam, p = _fast_accel_scenes()[name]()
    assert desc.contents.flags == ffi.VK_SCENE_FAST_ACCEL
    ds = DeviceScene(desc)
    try:
        _check_against_a(ds, desc, cam, p, oracle)
    finally:
        ds.close()


def test_both_kernel_instances_are_rendered(device, oracle):
    """aov_kernel<0> for a world of spheres only, aov_kernel<VKF_ALL_SCENE> for anything else (vk_api.hip enqueue_aov): by the scenes'
    features, since the launch log is vk_render's and first-hit calls leave it alone"""
    seen = set()
    for name in ("random_spheres_iow", "cornell_box"):
        hs, desc, cam, p = named(name)
        ds = DeviceScene(desc)
        try:
            seen.add(ds.info().features == 0)
            _check_against_a(ds, desc, cam, p, oracle)
        finally:
            ds.close()
    assert seen == {False, True}


@pytest.mark.parametrize("name", sorted(shared.DROPPED))
def test_dropped_samples_count_in_n_only(name, device, oracle):
    """samples with a non-finite albedo (NaN / infinite texture components on Lambertian spheres and on a phase function) add to no sum
    and not to hits, but count in n: a multi-sample window against the aggregate of the single-sample calls, bit for bit, with pixels
    whose coverage is below 1 because of the drop alone"""
    keep, desc, cam, p = shared.DROPPED[name]()
    n = p.samples_per_pixel
    ds = DeviceScene(desc)
    try:
        assert (ds.info().features == 0) == (name == "dropped_spheres")
        one = singles(ds, cam, p, range(n))
        window, st = ds.render_aov(cam, p)
        ref = aov_ref.ref_a(oracle, desc, cam, p, list(range(n)))
        print("\n   dropped samples, pixels partly dropped:", shared.check_dropped_window(name, p, one, window, ref))
    finally:
        ds.close()


@pytest.mark.parametrize("name", ("final_scene", "final_scene_nextweek"))
def test_media_scene_albedo_against_substitution(name, device, oracle):
    hs, desc, cam, p = named(name, width=16)
    ds = DeviceScene(desc)
    try:
        _check_against_b(ds, desc, cam, p, oracle)
    finally:
        ds.close()


_fog_scene = shared.fog_scene


def test_same_first_hit_as_the_radiance_sample(device):
    keep, desc, emit = _fog_scene()
    cam = camera((0, 0, 10), (0, 0, 0), vfov=30.0)
    p = params(16, 16, 8, max_depth=1, seed=11, integrator=ffi.VK_INTEGRATOR_SCATTER)
    ds = DeviceScene(desc)
    try:
        lib = ds._lib
        lib.vk_debug_render_samples.restype = C.c_int
        lib.vk_debug_render_samples.argtypes = [C.c_void_p, C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_void_p, C.c_void_p]
        img = np.zeros((16, 16, 3), f32)
        dump = np.zeros((16 * 16 * 8, 4), f32)
        assert lib.vk_debug_render_samples(ds._h, C.byref(cam), C.byref(p), img.ctypes.data, dump.ctypes.data) == 0
        rad = dump[:, :3].reshape(16, 16, 8, 3)
        e = f32(emit)
        seen = set()
        for s, g in enumerate(singles(ds, cam, p, range(8))):
            on_back = (g["albedo"] == e).all(-1)
            np.testing.assert_array_equal((rad[:, :, s] == e).all(-1), on_back)
            seen |= set(np.unique(on_back).tolist())
        assert seen == {False, True}           # both kinds of first hit occur
    finally:
        ds.close()


def test_medium_coverage_statistics(device):
    d = Desc()
    rho, R = 0.7, 1.0
    world = d.medium(d.sphere((0, 0, 0), R, d.lambertian(0.5, 0.5, 0.5)), rho, d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(0.5, 0.5, 0.5)))
    desc = d.finish(world)
    cam = camera((0, 0, 0), (0, 0, -1), vfov=60.0)            # inside: every ray runs R - 0.001 |d| through the medium
    p = params(16, 16, 256, seed=3, integrator=ffi.VK_INTEGRATOR_SCATTER)
    ds = DeviceScene(desc)
    try:
        out, st = ds.render_aov(cam, p, want=("coverage",))
        assert st.samples == 16 * 16 * 256
        xs, ys = np.meshgrid(np.arange(16) + 0.5, np.arange(16) + 0.5)
        dd = (np.array(list(cam.lower_left_corner))[None, None] + np.array(list(cam.horizontal)) * (xs / 15.0)[..., None]
              + np.array(list(cam.vertical)) * (ys / 15.0)[..., None] - np.array(list(cam.origin)))
        L = R - 0.001 * np.linalg.norm(dd, axis=-1)
        pk = 1.0 - np.exp(-rho * L)
        n = 256
        hits = (out["coverage"].astype(np.float64) * n).round()
        sigma = np.sqrt((n * pk * (1 - pk)).sum())
        assert abs(hits.sum() - (n * pk).sum()) < 5 * sigma, (hits.sum(), (n * pk).sum(), sigma)
    finally:
        ds.close()


def test_windows_aggregate_exactly(device):
    hs, desc, cam, p = named("cornell_box", width=16)
    ds = DeviceScene(desc)
    try:
        one = singles(ds, cam, p, range(24))
        for lo, hi in ((0, 16), (8, 24)):
            q = hs.params(16, hi - lo, 50, seed=7, height=16)
            got, st = ds.render_aov(cam, q, first_sample=lo)
            want = aov_ref.aggregate(one[lo:hi])
            for ch in aov_ref.CHANNELS:
                np.testing.assert_array_equal(got[ch].view(np.uint32), want[ch].view(np.uint32), err_msg=ch)
    finally:
        ds.close()


def test_call_shapes_are_bit_identical(device):
    import torch
    hs, desc, cam, _ = named("cornell_box")
    p = hs.params(40, 4, 50, seed=9, height=28)
    ds = DeviceScene(desc)
    multi = DeviceScene(desc, devices=[0, 0])
    try:
        full, st = ds.render_aov(cam, p, first_sample=5)
        assert st.kernel_launches == 1 and st.clamped_samples == 0 and st.samples == 40 * 28 * 4
        # the device call
        bufs = {ch: torch.zeros(v.shape, dtype=torch.float32, device="cuda:0") for ch, v in full.items()}
        ds.render_aov_device(cam, p, 5, bufs["albedo"].data_ptr(), bufs["normal"].data_ptr(), bufs["depth"].data_ptr(),
                             bufs["coverage"].data_ptr())
        torch.cuda.synchronize()
        for ch in full:
            np.testing.assert_array_equal(bufs[ch].cpu().numpy().view(np.uint32), full[ch].view(np.uint32), err_msg=ch)
        # each channel alone
        for ch in full:
            alone, _ = ds.render_aov(cam, p, first_sample=5, want=(ch,))
            np.testing.assert_array_equal(alone[ch].view(np.uint32), full[ch].view(np.uint32), err_msg=ch)
        # tile partitions: a NaN sentinel outside, the union is the whole image
        union = {ch: np.full_like(v, np.nan) for ch, v in full.items()}
        tile_of = (np.arange(28)[:, None] // 8) * 5 + (np.arange(40)[None, :] // 8)
        for rank in range(3):
            q = hs.params(40, 4, 50, seed=9, height=28, tile_rank=rank, tile_world=3)
            part, _ = ds.render_aov(cam, q, first_sample=5, out={ch: np.full_like(v, np.nan) for ch, v in full.items()})
            mine = tile_of % 3 == rank
            for ch in full:
                assert np.isnan(part[ch][~mine]).all(), ch
                union[ch][mine] = part[ch][mine]
        for ch in full:
            np.testing.assert_array_equal(union[ch].view(np.uint32), full[ch].view(np.uint32), err_msg=ch)
        # a multi-device scene: on devices[0]
        m, _ = multi.render_aov(cam, p, first_sample=5)
        for ch in full:
            np.testing.assert_array_equal(m[ch].view(np.uint32), full[ch].view(np.uint32), err_msg=ch)
    finally:
        multi.close()
        ds.close()


def test_render_is_not_disturbed(device):
    hs, desc, cam, _ = named("random_spheres_iow")
    p = hs.params(64, 16, 50, seed=4, height=48)
    ds = DeviceScene(desc)
    try:
        from vecchio_amd import ffi as F
        launches = lambda: [bytes(x) for x in F.last_launches(ds._lib, ds._h)]
        a, sa = ds.render(cam, p)
        la, ra = launches(), ds.last_requeued_samples()
        ds.render_aov(cam, hs.params(64, 4, 50, seed=4, height=48))
        # what describes the last frame is still the first frame's
        assert launches() == la
        b, sb = ds.render(cam, p)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        assert launches() == la and ds.last_requeued_samples() == ra
        assert sb.clamped_samples == sa.clamped_samples
        # a progress handle interrupted by an AOV call
        with ds.progress(cam, p) as pr:
            pr.step(6)
            ds.render_aov(cam, hs.params(64, 2, 50, seed=4, height=48), first_sample=3)
            img, _ = pr.step(10)
        np.testing.assert_array_equal(img.view(np.uint32), a.view(np.uint32))
    finally:
        ds.close()


def test_invalid_calls_leave_buffers_untouched(device):
    hs, desc, cam, _ = named("cornell_box", width=16)
    ds = DeviceScene(desc)
    lib = ds._lib
    try:
        sentinel = np.full((16, 16, 3), 7.0, f32)
        cases = []
        q = hs.params(16, 2, 50, height=16, output_format=ffi.VK_OUTPUT_RGB8); cases.append((q, 0, cam))
        q = hs.params(16, 2, 50, height=16); q.samples_per_pixel = 0; cases.append((q, 0, cam))
        cases.append((hs.params(16, 2, 50, height=16), 0xFFFFFFFF - 1, cam))
        cases.append((hs.params(16, 2, 50, height=1), 0, cam))
        q = hs.params(1, 2, 50, height=16); cases.append((q, 0, cam))
        bad_cam = ffi.Camera(); C.pointer(bad_cam)[0] = cam; bad_cam.time1 = bad_cam.time0; cases.append((hs.params(16, 2, 50, height=16), 0, bad_cam))
        for q, first, c in cases:
            buf = sentinel.copy()
            st = lib.vk_render_aov(ds._h, C.byref(c), C.byref(q), first, buf.ctypes.data, None, None, None, None)
            assert st == ffi.VK_ERR_BAD_ARG, (st, lib.vk_last_error())
            np.testing.assert_array_equal(buf, sentinel)
        q = hs.params(16, 2, 50, height=16)
        assert lib.vk_render_aov(ds._h, C.byref(cam), C.byref(q), 0, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
        assert lib.vk_render_aov_device(ds._h, C.byref(cam), C.byref(q), 0, None, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
    finally:
        ds.close()


def _read_pfm(path):
    raw = path.read_bytes()
    head, rest = raw.split(b"\n", 3)[:3], raw.split(b"\n", 3)[3]
    kind, (w, h), scale = head[0], map(int, head[1].split()), float(head[2])
    ch = 3 if kind == b"PF" else 1
    assert kind in (b"PF", b"Pf") and scale == -1.0 and len(rest) == w * h * ch * 4, (kind, w, h, scale, len(rest))
    a = np.frombuffer(rest, dtype="<f4").reshape(h, w, ch)
    return a if ch == 3 else a[..., 0]


def test_cli_writes_the_pfm_buffers(device, tmp_path):
    import subprocess
    from vecchio_amd import build
    cli = build.build_cli()
    a, b = tmp_path / "plain", tmp_path / "aov"
    a.mkdir()
    b.mkdir()
    subprocess.run([cli, "cornell_box", "64", "16", "10", "1", "1", "1"], cwd=a, check=True, timeout=300, capture_output=True)
    subprocess.run([cli, "cornell_box", "64", "16", "10", "1", "1", "1", "4"], cwd=b, check=True, timeout=300, capture_output=True)
    assert (a / "output_0000.ppm").read_bytes() == (b / "output_0000.ppm").read_bytes()
    names = ["output_0000.pfm"] + [f"output_0000_{ch}.pfm" for ch in aov_ref.CHANNELS]
    assert sorted(f.name for f in b.iterdir()) == sorted(["output_0000.ppm"] + names)
    hs = HostScene("cornell_box", 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        img, _ = ds.render(cam, hs.params(64, 16, 10, seed=2))
        np.testing.assert_array_equal(_read_pfm(b / "output_0000.pfm"), img)
        got, _ = ds.render_aov(cam, hs.params(64, 4, 10, seed=2))
        for ch in aov_ref.CHANNELS:
            np.testing.assert_array_equal(_read_pfm(b / f"output_0000_{ch}.pfm").view(np.uint32), got[ch].view(np.uint32), err_msg=ch)
    finally:
        ds.close()
