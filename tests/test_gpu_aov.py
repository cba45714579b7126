"""First-hit buffers (vk_render_aov) on the MI355X: per sample against the two oracle references of tests/aov_ref.py, the same first hit as
the radiance sample, medium statistics, exact aggregation, every call shape bit for bit, non-interference with vk_render and progress
handles, invalid calls."""
import ctypes as C

import numpy as np
import pytest

import aov_ref
from descs import Desc, camera, params
from test_fuzz_scenes import Gen
from vecchio_amd import DeviceScene, HostScene, ffi

pytestmark = pytest.mark.gpu

f32 = np.float32
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


def media_free(desc):
    return desc.contents.n_media == 0


def _check_against_a(ds, desc, cam, p, oracle, samples=(0, 1)):
    got = singles(ds, cam, p, samples)
    ref = aov_ref.ref_a(oracle, desc, cam, p, list(samples))
    for k, g in enumerate(got):
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


@pytest.mark.parametrize("seed", [2, 3, 4, 6, 8, 9])      # the media-free graphs among tests/test_fuzz_scenes.py Gen(1000 + 0..11)
def test_fuzz_graph_per_sample_against_oracle(seed, device, oracle):
    g, desc, cam, p = fuzz(seed)
    assert media_free(desc)
    ds = DeviceScene(desc)
    try:
        _check_against_a(ds, desc, cam, p, oracle)
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


def _fog_scene():
    d = Desc()
    emit = (0.3, 0.6, 0.9)
    back = d.xy_rect(-20, 20, -20, 20, -5.0, d.light(*emit))
    fog = d.medium(d.sphere((0, 0, 0), 2.0, d.lambertian(0.5, 0.5, 0.5)), 0.4, d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(0.8, 0.2, 0.2)))
    world = d.big_box(fog, back)
    return d, d.finish(world), emit


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
