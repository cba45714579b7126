"""-m gpu: guided upsampling (vk_upsample_*) on the MI355X.  RESTATEMENT: the device's frame, stderr3 and the two counts equal the host
build of vk_upsample.h over every case of upsample_cases.cases() and tests/upsample_ref.py over a spread of them (the CPU suite holds the
two equal on all), bit for bit (a NaN's payload aside), in the PLAIN, TILED and AUTO forms — 2x2->2x2, 2x2->5x5, 7x5->16x11, 9x7->9x7,
33x9->65x17 (one pixel past a 32 x 8 tile each way), 31x23->130x70, 64x36->256x144, 100x75->317x301 and a many-tile frame,
321x181->641x361.  AUTO's rule.  EQUIVALENCE of the host-pointer and device routes, a second apply without a reload, a changed floor's
re-prepare.  A RENDERED Cornell box, 64x64 -> 128x128, through vk_denoise and vk_tone; the command-line tool's scale argument.  Refusals
on a live handle, non-interference with vk_render, and the live-object count."""
import ctypes as C

import numpy as np
import pytest

import emu_upsample_ffi as EMU
import upsample_cases as K
import upsample_ref as R
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMS = (ffi.VK_UPSAMPLE_FORM_PLAIN, ffi.VK_UPSAMPLE_FORM_TILED, ffi.VK_UPSAMPLE_FORM_AUTO)
SIZES = [(2, 2, 2, 2), (2, 2, 5, 5), (7, 5, 16, 11), (9, 7, 9, 7), (33, 9, 65, 17), (31, 23, 130, 70), (64, 36, 256, 144),
         (100, 75, 317, 301), (321, 181, 641, 361)]
# the cases the numpy restatement is run on as well (it takes a second a case on the largest frame)
REF_CASES = ("ganz-se1", "g0-se0", "gz-se1", "block", "floor", "s0.5-q3")


def auto_form(w, h, W, H):
    """AUTO's documented rule (DESIGN.md "Guided upsampling"), a function of the sizes only: the tiled form everywhere — it was
    measured faster in all six cells of the report, and nothing smaller was measured"""
    return ffi.VK_UPSAMPLE_FORM_TILED


@pytest.fixture(scope="module")
def scene(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    yield ds
    ds.close()


def differing(a, b):
    return np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:4].tolist()


def load_and_apply(u, fr, g, se, pkw):
    kw = K.arguments(fr, g, se)
    u.load(fr["color"], kw.get("stderr3"), kw.get("albedo"), kw.get("normal"), kw.get("depth"))
    return u.apply(kw.get("albedo_hi"), kw.get("normal_hi"), kw.get("depth_hi"), want_stderr=se, **pkw)


# ---------------------------------------------------------------- 1. the restatement, the counts and AUTO's rule
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d-%dx%d" % s for s in SIZES])
def test_device_equals_the_restatement_and_the_host_build(size, scene, emu):
    w, h, W, H = size
    names = [c[0] for c in K.cases()]
    assert set(REF_CASES) <= set(names)
    applies = 0
    with scene.upsample(w, h, W, H) as u:
        assert EMU.auto_form(*size) == auto_form(*size)
        for name, fkw, g, se, pkw in K.cases():
            fr = K.frame(w, h, W, H, **fkw)
            kw = dict(K.arguments(fr, g, se), **pkw)
            want = EMU.apply(fr["color"], W, H, **kw)
            if name in REF_CASES:
                ref = R.apply(fr["color"], W, H, **kw)
                assert K.same(ref[0], want[0]) and K.same(ref[1], want[1]) and ref[2:] == want[2:], (size, name)
            for form in FORMS:
                u.set_form(form)
                out, err = load_and_apply(u, fr, g, se, pkw)
                applies += 1
                assert K.same(out, want[0]), (size, name, form, differing(out, want[0]))
                assert K.same(err, want[1]), (size, name, form)
                info = u.info()
                assert (info.fallback_pixels, info.empty_pixels) == want[2:], (size, name, form, info.fallback_pixels, info.empty_pixels, want[2:])
                assert info.last_form == (form or auto_form(*size)), (size, name, form)
                bits = (1 if se else 0) | (2 if "a" in g else 0) | (4 if "n" in g else 0) | (8 if "z" in g else 0)
                assert info.guides == bits and info.loaded == 1
        ms = u.last_ms()
        info = u.info()
        assert np.isfinite(ms) and ms >= 0 and info.last_kernel_ms == ms and info.applies == applies and info.loads == applies
        assert (info.width_lo, info.height_lo, info.width_hi, info.height_hi) == size


# ---------------------------------------------------------------- 2. routes, a second apply, a changed floor
def test_routes_a_second_apply_and_a_changed_floor(scene, emu):
    import torch
    w, h, W, H = 31, 23, 130, 70
    fr = K.frame(w, h, W, H, seed=7, bad=True)
    kw = K.arguments(fr, "anz", True)
    first = EMU.apply(fr["color"], W, H, **kw)
    second = EMU.apply(fr["color"], W, H, sigma_z=4.0, normal_squarings=2, **kw)
    floored = EMU.apply(fr["color"], W, H, albedo_floor=0.3, **kw)
    no_depth = EMU.apply(fr["color"], W, H, **{k: v for k, v in kw.items() if k != "depth_hi"})
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, f32)).cuda()
    with scene.upsample(w, h, W, H) as u:
        for form in FORMS:
            u.set_form(form)
            u.load(fr["color"], fr["stderr3"], fr["albedo"], fr["normal"], fr["depth"])
            out, err = u.apply(fr["albedo_hi"], fr["normal_hi"], fr["depth_hi"])
            assert K.same(out, first[0]) and K.same(err, first[1]) and u.info().last_launches == 1
            # the device route: tensors in, the caller's low buffers free after the load
            lo = [dev(fr[k]) for k in ("color", "stderr3", "albedo", "normal", "depth")]
            hi = [dev(fr[k]) for k in ("albedo_hi", "normal_hi", "depth_hi")]
            u.load_device(*lo)
            torch.cuda.synchronize()
            for t in lo:
                t.fill_(float("nan"))
            d_out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
            d_err = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
            assert u.apply_device(d_out, d_err, *hi) == (d_out, d_err)
            assert u.last_ms() >= 0                                                # (waits for the event behind the filter)
            torch.cuda.synchronize()
            assert K.same(d_out.cpu().numpy(), first[0]) and K.same(d_err.cpu().numpy(), first[1]), form
            # a second apply with other parameters, bare pointers, no reload
            loads = u.info().loads
            u.apply_device(d_out.data_ptr(), d_err.data_ptr(), *[t.data_ptr() for t in hi], sigma_z=4.0, normal_squarings=2)
            torch.cuda.synchronize()
            assert K.same(d_out.cpu().numpy(), second[0]) and K.same(d_err.cpu().numpy(), second[1]) and u.info().loads == loads
            # a depth on one side only switches the term off
            out, err = u.apply(fr["albedo_hi"], fr["normal_hi"], None)
            assert K.same(out, no_depth[0]) and K.same(err, no_depth[1]) and (u.info().fallback_pixels, u.info().empty_pixels) == no_depth[2:]
            # another floor: the planes are prepared again from the handle's copy (two launches), and once more on the way back
            out, err = u.apply(fr["albedo_hi"], fr["normal_hi"], fr["depth_hi"], albedo_floor=0.3)
            assert K.same(out, floored[0]) and K.same(err, floored[1]) and u.info().last_launches == 2
            out, _ = u.apply(fr["albedo_hi"], fr["normal_hi"], fr["depth_hi"], albedo_floor=0.3, want_stderr=False)
            assert K.same(out, floored[0]) and u.info().last_launches == 1
            out, err = u.apply(fr["albedo_hi"], fr["normal_hi"], fr["depth_hi"])
            assert K.same(out, first[0]) and K.same(err, first[1]) and u.info().last_launches == 2
        assert not K.same(first[0], second[0]) and not K.same(first[0], floored[0]) and not K.same(first[0], no_depth[0])


# ---------------------------------------------------------------- 3. a rendered frame, upsampled, denoised and encoded
def test_rendered_cornell_upsampled_denoised_and_encoded(scene, host_scenes, emu):
    hs, cam = host_scenes("cornell_box")
    lo_p, hi_p = hs.params(64, 16, 12, seed=3, height=64), hs.params(128, 4, 12, seed=3, height=128)
    with scene.progress(cam, lo_p, stderr=True) as pr:
        for _ in range(4):
            color, _ = pr.step(4)
        se = pr.stderr()
    color = np.ascontiguousarray(color, f32)
    lo, _ = scene.render_aov(cam, hs.params(64, 4, 12, seed=3, height=64), want=("albedo", "normal", "depth"))
    hi, _ = scene.render_aov(cam, hi_p, want=("albedo", "normal", "depth"))
    want = R.apply(color, 128, 128, stderr3=se, albedo=lo["albedo"], normal=lo["normal"], depth=lo["depth"], albedo_hi=hi["albedo"],
                   normal_hi=hi["normal"], depth_hi=hi["depth"])
    with scene.upsample(64, 64, 128, 128) as u:
        for form in FORMS:
            u.set_form(form)
            u.load(color, se, lo["albedo"], lo["normal"], lo["depth"])
            out, err = u.apply(hi["albedo"], hi["normal"], hi["depth"])
            assert K.same(out, want[0]) and K.same(err, want[1]) and (u.info().fallback_pixels, u.info().empty_pixels) == want[2:]
    assert np.isfinite(out).all() and np.isfinite(err).all() and (err >= 0).all() and want[3] == 0
    # the frame is the low one, enlarged: close to it on average, and a frame that vk_denoise and vk_tone take
    assert abs(float(out.mean()) / float(color.mean()) - 1) < 0.05
    clean, _ = scene.denoise(out, err, hi["albedo"], hi["normal"], hi["depth"])
    assert clean.shape == (128, 128, 3) and np.isfinite(clean).all()
    with scene.tone(128, 128) as t:
        t.load(clean)
        t.meter()
        codes = t.encode()
    assert codes.shape[:2] == (128, 128) and 0 < int(codes.min()) + 1 and int(codes.max()) <= 255 and len(np.unique(codes)) > 16


# ---------------------------------------------------------------- 4. refusals that need a handle, and what a handle owns
def test_refusals_with_a_handle_and_live_objects(device, host_scenes):
    dbg = ffi.load_debug_lib()
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc, lib=dbg)

    def live():
        out = (C.c_uint64 * 4)()
        assert dbg.vk_debug_live_objects(C.byref(out)) == ffi.VK_OK
        return tuple(out)

    try:
        before = live()
        w, h, W, H = 9, 7, 31, 23
        u = ds.upsample(w, h, W, H)
        assert live()[0] == before[0] + 3 and live()[2] == before[2] + 2             # the copy, the planes, the counts; two events
        own = w * h * 13 * 4 + w * h * 48 + 8
        info = u.info()
        assert info.scratch_bytes == own and (info.applies, info.loads, info.loaded, info.guides, info.last_form) == (0, 0, 0, 0, 0)
        assert info.last_kernel_ms == 0 and (info.fallback_pixels, info.empty_pixels) == (0, 0)
        fr = K.frame(w, h, W, H, seed=2)
        out, se = np.full((H, W, 3), 7, f32), np.full((H, W, 3), 7, f32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)
        ok = u.params()

        def refused(word, p=ok, albedo=None, want_se=False):
            rc = dbg.vk_upsample_apply(u._h, C.byref(p), ptr(albedo) if albedo is not None else None, None, None, ptr(out), ptr(se) if want_se else None)
            assert rc == ffi.VK_ERR_BAD_ARG and word in dbg.vk_last_error(), (word, dbg.vk_last_error())
            assert (out == 7).all() and (se == 7).all()

        refused(b"vk_upsample_apply before vk_upsample_load")
        u.load(fr["color"])
        assert u.info().guides == 0 and u.info().loaded == 1
        refused(b"albedo must be given at both sizes or at neither", albedo=fr["albedo_hi"])
        refused(b"stderr3_out wanted but no stderr3 was loaded", want_se=True)
        u.load(fr["color"], fr["stderr3"], fr["albedo"])
        assert u.info().guides == 3
        refused(b"albedo must be given at both sizes or at neither")
        refused(b"sigma_z must be finite and > 0", u.params(sigma_z=0.0), fr["albedo_hi"])
        refused(b"sigma_z must be finite and > 0", u.params(sigma_z=float("nan")), fr["albedo_hi"])
        refused(b"normal_squarings must be in 0..10", u.params(normal_squarings=11), fr["albedo_hi"])
        refused(b"albedo_floor must be finite and > 0", u.params(albedo_floor=float("inf")), fr["albedo_hi"])
        refused(b"unknown upsample flags", u.params(flags=1), fr["albedo_hi"])
        refused(b"unknown upsample flags", u.params(_pad=2), fr["albedo_hi"])
        assert dbg.vk_upsample_apply(u._h, C.byref(ok), ptr(fr["albedo_hi"]), None, None, None, None) == ffi.VK_ERR_BAD_ARG
        assert dbg.vk_upsample_apply_device(u._h, C.byref(ok), None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
        assert dbg.vk_upsample_load(u._h, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG and u.info().loads == 2
        assert u.info().applies == 0 and live()[0] == before[0] + 3
        got = u.apply(fr["albedo_hi"], normal_squarings=10)                             # 10 squarings are admitted
        want = R.apply(fr["color"], W, H, stderr3=fr["stderr3"], albedo=fr["albedo"], albedo_hi=fr["albedo_hi"], normal_squarings=10)
        assert K.same(got[0], want[0]) and K.same(got[1], want[1])
        assert live()[0] == before[0] + 4                                               # the high guide and the frames out, on the first host apply
        assert u.info().scratch_bytes == own + 3 * W * H * 12 and u.info().applies == 1
        u.reset()
        assert u.info().loaded == 0 and u.info().guides == 0
        refused(b"vk_upsample_apply before vk_upsample_load")
        assert dbg.vk_debug_upsample_set_form(u._h, 3) == ffi.VK_ERR_BAD_ARG and b"unknown upsample form" in dbg.vk_last_error()
        u.close()
        assert live() == before
        dbg.vk_upsample_destroy(None)
    finally:
        ds.close()


# ---------------------------------------------------------------- 5. non-interference
def test_leaves_renders_alone(scene, host_scenes):
    hs, cam = host_scenes("cornell_box")
    ds = scene
    p = hs.params(32, 16, 12, seed=4)
    launches = lambda: [bytes(x) for x in ffi.last_launches(ds._lib, ds._h)]
    a, sa = ds.render(cam, p)
    la, ra, ms = launches(), ds.last_requeued_samples(), ds.last_kernel_ms()
    fr = K.frame(24, 20, 48, 40, seed=9)
    with ds.upsample(24, 20, 48, 40) as u:
        for form in FORMS:
            u.set_form(form)
            load_and_apply(u, fr, "anz", True, {})
        assert launches() == la and ds.last_requeued_samples() == ra and ds.last_kernel_ms() == ms
    b, sb = ds.render(cam, p)
    assert K.same(b, a) and launches() == la and sb.clamped_samples == sa.clamped_samples


# ---------------------------------------------------------------- 6. the command-line tool's scale argument
def test_cli_scale_argument(device, host_scenes, tmp_path, emu):
    import subprocess
    from test_gpu_aov import _read_pfm
    from vecchio_amd import build
    cli = build.build_cli()
    # (aov_spp = 2 writes the float frames; steps = 1: no standard error)
    base = ["cornell_box", "64", "8", "12", "1", "1", "1", "2", "0", "0", "0", "0", "0"]
    dirs = {}
    for key, extra in (("absent", []), ("off", ["100"]), ("half", ["50"])):
        dirs[key] = tmp_path / key
        dirs[key].mkdir()
        subprocess.run([cli] + base + extra, cwd=dirs[key], check=True, timeout=300, capture_output=True)
    names = sorted(f.name for f in dirs["absent"].iterdir())
    assert sorted(f.name for f in dirs["off"].iterdir()) == names
    for n in names:
        assert (dirs["absent"] / n).read_bytes() == (dirs["off"] / n).read_bytes(), n
    new = ["output_0000_lo_albedo.pfm", "output_0000_lo_normal.pfm", "output_0000_lo_depth.pfm", "output_0000_upsampled.pfm",
           "output_0000_upsampled.ppm"]
    assert sorted(f.name for f in dirs["half"].iterdir()) == sorted(names + new)
    rd = lambda n: _read_pfm(dirs["half"] / f"output_0000{n}.pfm")
    low = rd("")
    assert low.shape[:2] == (32, 32) and rd("_albedo").shape[:2] == (64, 64)
    # the full-size first-hit buffers are the ones a plain run writes
    for n in ("_albedo", "_normal", "_depth", "_coverage"):
        assert (dirs["absent"] / f"output_0000{n}.pfm").read_bytes() == (dirs["half"] / f"output_0000{n}.pfm").read_bytes(), n
    want = EMU.apply(low, 64, 64, albedo=rd("_lo_albedo"), normal=rd("_lo_normal"), depth=rd("_lo_depth"), albedo_hi=rd("_albedo"),
                     normal_hi=rd("_normal"), depth_hi=rd("_depth"), want_stderr=False)
    assert K.same(rd("_upsampled"), want[0])
    bad = subprocess.run([cli] + base[:7] + ["0", "0", "0", "0", "0", "0", "50"], cwd=tmp_path, capture_output=True, timeout=60)
    assert bad.returncode == 2 and b"aov_spp > 0" in bad.stderr
