"""-m gpu: the denoiser (vk_denoise) on the MI355X, bit for bit against the numpy restatement of its definition (tests/denoise_ref.py) on
synthetic and rendered inputs; the plain and the staged form of the level kernel; every call shape; vk_progress_stderr_device against the
host call; non-interference with vk_render and progress handles; invalid calls; the CLI; and the end-to-end improvement of a Cornell frame."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import denoise_ref as R
from vecchio_amd import DeviceScene, HostScene, build, ffi

pytestmark = pytest.mark.gpu

f32 = np.float32
GUIDES = ("stderr3", "albedo", "normal", "depth")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what=""):
    """bit-identical, NaNs aside (an invalid pixel's NaN comes back as it went in: compared as bits too)"""
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} pixels differ, first at {np.argwhere(bad.any(-1))[:3].tolist()}"


_ds = {}


def scene(name="cornell_box", **kw):
    key = (name, tuple(sorted(kw.items(), key=str)))
    if key not in _ds:
        hs = HostScene(name, 1)
        _ds[key] = (hs, hs.next_camera(), DeviceScene(hs.desc, **{k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}))
    return _ds[key]


def run(ds, g, form=None, **over):
    h, w = g["color"].shape[:2]
    dp = ds.denoise_params(w, h, **over)
    if form is not None:
        assert ds._lib.vk_debug_denoise_form(ds._h, form) == ffi.VK_OK
    try:
        out, st = ds.denoise(g["color"], g.get("stderr3"), g.get("albedo"), g.get("normal"), g.get("depth"), params=dp)
    finally:
        if form is not None:
            ds._lib.vk_debug_denoise_form(ds._h, ffi.VK_DENOISE_FORM_AUTO)
    assert st.samples == w * h and st.kernel_launches == 1 + dp.levels and st.kernel_ms > 0
    return out


def ref(g, **over):
    kw = dict(R.DEFAULTS)
    kw.update(over)
    return R.denoise(g["color"], g.get("stderr3"), g.get("albedo"), g.get("normal"), g.get("depth"), **kw)


@pytest.mark.parametrize("width,height", [(1, 1), (3, 200), (37, 29), (256, 144)])
def test_synthetic_inputs_bit_for_bit(width, height, device):
    hs, cam, ds = scene()
    g = R.synthetic(width, height, seed=width)
    assert width * height < 12 or not np.isfinite(g["color"]).all()
    for levels in range(1, 9):                     # (spacing beyond the image included)
        same(run(ds, g, levels=levels), ref(g, levels=levels), f"{width}x{height}, {levels} levels")
    same(run(ds, g, normal_squarings=0, sigma_l=0.7, sigma_z=3.0, albedo_floor=0.25),
         ref(g, normal_squarings=0, sigma_l=0.7, sigma_z=3.0, albedo_floor=0.25), "other parameters")


def test_every_combination_of_the_optional_inputs(device):
    hs, cam, ds = scene()
    g = R.synthetic(37, 29, seed=2)
    outs = set()
    for keep in itertools.product((False, True), repeat=4):
        sub = {"color": g["color"], **{k: g[k] for k, on in zip(GUIDES, keep) if on}}
        got = run(ds, sub, levels=4)
        same(got, ref(sub, levels=4), str(keep))
        outs.add(got.tobytes())
    assert len(outs) == 16                         # every term does something


@pytest.mark.parametrize("width,height", [(37, 29), (256, 144), (200, 3)])
def test_plain_and_staged_forms_agree_at_every_level(width, height, device):
    hs, cam, ds = scene()
    g = R.synthetic(width, height, seed=7)
    for levels in range(1, 9):
        plain = run(ds, g, form=ffi.VK_DENOISE_FORM_PLAIN, levels=levels)
        staged = run(ds, g, form=ffi.VK_DENOISE_FORM_STAGED, levels=levels)
        auto = run(ds, g, levels=levels)
        same(staged, plain, f"staged vs plain, {levels} levels")
        same(auto, plain, f"auto vs plain, {levels} levels")


def rendered(name, width, height, spp=16, windows=4, sky=False):
    """the noisy mean, its standard error and the AOVs of a frame rendered in `windows` windows"""
    hs, cam, ds = scene(name)
    p = hs.params(width, spp, 50, seed=5, height=height)
    with ds.progress(cam, p, stderr=True) as pr:
        for _ in range(windows):
            img, _ = pr.step(spp // windows)
        se = pr.stderr()
    aov, _ = ds.render_aov(cam, p)
    return dict(color=img.copy(), stderr3=se, albedo=aov["albedo"], normal=aov["normal"], depth=aov["depth"])


@pytest.mark.parametrize("name,width,height", [("cornell_box", 64, 64), ("random_spheres_iow", 64, 48)])
def test_rendered_inputs_bit_for_bit(name, width, height, device):
    hs, cam, ds = scene(name)
    g = rendered(name, width, height)
    if name == "random_spheres_iow":
        assert np.isinf(g["depth"]).any()          # sky
    got = run(ds, g)
    same(got, ref(g), name)
    assert (got != g["color"]).any()


def test_call_shapes_and_scratch_regrowth(device):
    import torch
    hs, cam, ds = scene()
    big, small = R.synthetic(256, 144, seed=1), R.synthetic(37, 29, seed=1)
    first = run(ds, big)
    s = run(ds, small)
    same(s, ref(small), "small after large")
    same(run(ds, big), first, "large again")
    # the device call
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in big.items()}
    out = torch.full((144, 256, 3), 7.0, dtype=torch.float32, device="cuda:0")
    ds.denoise_device(ds.denoise_params(256, 144), dev["color"].data_ptr(), out.data_ptr(), dev["stderr3"].data_ptr(),
                      dev["albedo"].data_ptr(), dev["normal"].data_ptr(), dev["depth"].data_ptr())
    torch.cuda.synchronize()
    same(out.cpu().numpy(), first, "device call")
    # a multi-device scene: on devices[0]
    _, _, multi = scene("cornell_box", devices=(0, 0))
    same(run(multi, big), first, "multi-device scene")


def test_stderr_device_matches_the_host_call(device):
    import torch
    hs, cam, ds = scene("random_spheres_iow")

    def both(pr, w, h):
        host = pr.stderr()
        d = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda:0")
        pr.stderr_device(d.data_ptr())
        torch.cuda.synchronize()
        return host, d.cpu().numpy()

    p = hs.params(64, 64, 50, seed=3, height=48)
    with ds.progress(cam, p, stderr=True) as pr:                       # a plain handle
        pr.step(5)
        d = torch.zeros((48, 64, 3), dtype=torch.float32, device="cuda:0")
        assert ds._lib.vk_progress_stderr_device(pr._h, C.c_void_p(d.data_ptr()), None) == ffi.VK_ERR_BAD_ARG      # one step
        pr.step(7), pr.step(4)
        host, dev = both(pr, 64, 48)
        same(dev, host, "plain handle")
        assert (host > 0).any()
    with ds.progress(cam, p) as pr:                                    # no VK_PROGRESS_STDERR
        pr.step(4), pr.step(4)
        assert ds._lib.vk_progress_stderr_device(pr._h, C.c_void_p(d.data_ptr()), None) == ffi.VK_ERR_BAD_ARG
    # an adaptive handle with frozen tiles: each tile's own N and k
    with ds.progress(cam, p, stderr=True) as pr:
        for _ in range(4):
            pr.step(8)
        # (the median over the 6 x 8 tiles of the largest per-pixel standard error: freezes some tiles, not all)
        tol = float(np.median(pr.stderr().max(axis=2).reshape(6, 8, 8, 8).max(axis=(1, 3))))
    with ds.progress(cam, p, adaptive=dict(abs_tol=tol, rel_tol=0.0, min_samples=0, min_steps=2)) as pr:
        for _ in range(8):
            pr.step(8)
        tmap, inf = pr.tile_samples()
        assert 0 < inf.tiles_active < inf.tiles_total
        host, dev = both(pr, 64, 48)
        same(dev, host, "adaptive handle")
    # a partition: its pixels only, the NaN sentinel elsewhere
    q = hs.params(64, 64, 50, seed=3, height=48, tile_rank=1, tile_world=3)
    with ds.progress(cam, q, stderr=True) as pr:
        pr.step(6), pr.step(6)
        host = np.full((48, 64, 3), np.nan, f32)
        assert ds._lib.vk_progress_stderr(pr._h, host.ctypes.data_as(C.c_void_p)) == ffi.VK_OK
        _, dev = both(pr, 64, 48)
        same(dev, host, "partition")
        tile_of = (np.arange(48)[:, None] // 8) * 8 + (np.arange(64)[None, :] // 8)
        assert np.isnan(dev[tile_of % 3 != 1]).all() and np.isfinite(dev[tile_of % 3 == 1]).all()
    # a handle on a multi-device scene: the host call is the way
    _, _, multi = scene("random_spheres_iow", devices=(0, 0))
    with multi.progress(cam, p, stderr=True) as pr:
        pr.step(4), pr.step(4)
        assert multi._lib.vk_progress_stderr_device(pr._h, C.c_void_p(d.data_ptr()), None) == ffi.VK_ERR_UNSUPPORTED
        assert np.isfinite(pr.stderr()).all()


def test_render_is_not_disturbed(device):
    hs, cam, ds = scene("random_spheres_iow")
    p = hs.params(64, 16, 50, seed=4, height=48)
    g = R.synthetic(64, 48, seed=9)
    launches = lambda: [bytes(x) for x in ffi.last_launches(ds._lib, ds._h)]
    a, sa = ds.render(cam, p)
    la, ra, ms = launches(), ds.last_requeued_samples(), ds.last_kernel_ms()
    run(ds, g)
    assert launches() == la and ds.last_requeued_samples() == ra and ds.last_kernel_ms() == ms
    b, sb = ds.render(cam, p)
    same(b, a, "vk_render after a denoise call")
    assert launches() == la and ds.last_requeued_samples() == ra and sb.clamped_samples == sa.clamped_samples
    with ds.progress(cam, p) as pr:                # a progress handle interrupted by a denoise call
        pr.step(6)
        run(ds, g)
        img, _ = pr.step(10)
    same(img, a, "progress handle around a denoise call")


def test_invalid_calls_leave_out_untouched(device):
    hs, cam, ds = scene()
    lib = ds._lib
    g = R.synthetic(16, 16, seed=4, invalid=False)
    sentinel = np.full((16, 16, 3), 7.0, f32)
    bad = [dict(levels=0), dict(levels=9), dict(normal_squarings=11), dict(flags=1), dict(width=0), dict(height=0)]
    for field in ("sigma_l", "sigma_z", "albedo_floor"):
        bad += [{field: v} for v in (0.0, -1.0, float("nan"), float("inf"))]
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    for over in bad:
        dp = ds.denoise_params(16, 16)
        for k, v in over.items():
            setattr(dp, k, v)
        out = sentinel.copy()
        rc = lib.vk_denoise(ds._h, C.byref(dp), ptr(g["color"]), ptr(g["stderr3"]), None, None, None, ptr(out), None)
        assert rc == ffi.VK_ERR_BAD_ARG, (over, rc)
        np.testing.assert_array_equal(out, sentinel)
    dp = ds.denoise_params(16, 16)
    out = sentinel.copy()
    assert lib.vk_denoise(ds._h, C.byref(dp), None, None, None, None, None, ptr(out), None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_denoise(ds._h, None, ptr(g["color"]), None, None, None, None, ptr(out), None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_denoise(ds._h, C.byref(dp), ptr(g["color"]), None, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_denoise_device(ds._h, C.byref(dp), None, None, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
    np.testing.assert_array_equal(out, sentinel)
    alias = g["color"].copy()
    for k in range(5):                             # out aliasing an input, whichever
        args = [ptr(g["color"]), None, None, None, None]
        args[k] = ptr(alias)
        assert lib.vk_denoise(ds._h, C.byref(dp), *args, ptr(alias), None) == ffi.VK_ERR_BAD_ARG, k
    np.testing.assert_array_equal(alias, g["color"])
    assert lib.vk_debug_denoise_form(ds._h, 3) == ffi.VK_ERR_BAD_ARG


def _read_pfm(path):
    raw = path.read_bytes()
    head, rest = raw.split(b"\n", 3)[:3], raw.split(b"\n", 3)[3]
    (w, h) = map(int, head[1].split())
    assert head[0] == b"PF" and float(head[2]) == -1.0 and len(rest) == w * h * 12
    return np.frombuffer(rest, dtype="<f4").reshape(h, w, 3)


def test_cli_writes_the_denoised_frame(device, tmp_path):
    cli = build.build_cli()
    a, b = tmp_path / "eight", tmp_path / "nine"
    a.mkdir(), b.mkdir()
    base = [cli, "cornell_box", "64", "16", "10", "1", "1", "4", "16"]
    subprocess.run(base, cwd=a, check=True, timeout=300, capture_output=True)
    subprocess.run(base + ["1"], cwd=b, check=True, timeout=300, capture_output=True)
    names = sorted(f.name for f in a.iterdir())
    assert names == sorted(["output_0000.ppm", "output_0000.pfm"] + [f"output_0000_{ch}.pfm" for ch in ("albedo", "normal", "depth", "coverage")]
                           + [f"output_0000_step{k:02d}.ppm" for k in range(4)])
    assert sorted(f.name for f in b.iterdir()) == sorted(names + ["output_0000_denoised.ppm", "output_0000_denoised.pfm"])
    for n in names:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    # refused without the error estimate or the first-hit buffers
    for argv in ([cli, "cornell_box", "64", "16", "10", "1", "1", "1", "16", "1"], [cli, "cornell_box", "64", "16", "10", "1", "1", "4", "0", "1"]):
        r = subprocess.run(argv, cwd=tmp_path, timeout=300, capture_output=True)
        assert r.returncode != 0 and b"denoise" in r.stderr
    hs, cam, ds = scene()
    p = hs.params(64, 16, 10, seed=2)
    with ds.progress(cam, p, stderr=True) as pr:
        for _ in range(4):
            img, _ = pr.step(4)
        se = pr.stderr()
    aov, _ = ds.render_aov(cam, p)
    want, _ = ds.denoise(img, se, aov["albedo"], aov["normal"], aov["depth"])
    same(_read_pfm(b / "output_0000_denoised.pfm"), want, "CLI")
    host = ffi.load_host_lib()
    rgb8 = np.zeros((64, 64, 3), np.uint8)
    host.vkh_to_color(want.ctypes.data_as(C.c_void_p), 64, 64, rgb8.ctypes.data_as(C.c_void_p))
    ppm = (b / "output_0000_denoised.ppm").read_text().split()            # plain PPM: P3, width, height, 255, then the values
    assert ppm[:4] == ["P3", "64", "64", "255"]
    np.testing.assert_array_equal(np.array(ppm[4:], np.uint8).reshape(64, 64, 3), rgb8)


def rel_mse(img, truth):
    return float(np.mean((img.astype(np.float64) - truth) ** 2 / (truth.astype(np.float64) ** 2 + 1e-2)))


# tools/denoise_report.py measured the ratio relMSE(denoised) / relMSE(noisy) of this frame (Cornell 128x128, 16 spp in 4 windows, AOVs at
# 16 spp, defaults, against 8192 spp with another seed) as R_MEASURED; the denoised frame must keep at least half of that improvement —
# ratio <= 1 - (1 - r) / 2 — the margin covering the change of seed.  The run it came from: see R_MEASURED_RUN and DESIGN.md.
R_MEASURED = 0.0284       # relMSE 0.430318 -> 0.012235
R_MEASURED_RUN = "profiles/denoise/denoise_report.jsonl (tools/denoise_report.py --part quality --sweep, 1x MI355X): cornell_box 128x128, 16 spp"


def test_cornell_frame_improves(device):
    hs, cam, ds = scene()
    g = rendered("cornell_box", 128, 128)
    truth, _ = ds.render(cam, hs.params(128, 8192, 50, seed=77, height=128))
    noisy, clean = rel_mse(g["color"], truth), rel_mse(run(ds, g), truth)
    print(f"relMSE noisy {noisy:.5f} denoised {clean:.5f} ratio {clean / noisy:.4f}")
    assert clean < noisy                           # a denoiser that does not improve this frame is broken
    assert clean / noisy <= 1.0 - (1.0 - R_MEASURED) / 2.0, (clean / noisy, R_MEASURED)
