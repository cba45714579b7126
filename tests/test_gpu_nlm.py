"""-m gpu: non-local means (vk_nlm_*) on the MI355X.  RESTATEMENT: the device's out and stderr3_out equal tests/nlm_ref.py and the host
build of vk_nlm.h bit for bit (a NaN's payload aside) in the PLAIN, TILED and AUTO forms — the CPU test's sizes and (R, F) grid, with and
without albedo, the tile's boundaries (the tiled form's tile is 32 x 8, the plain form's workgroup 64 x 4: widths and heights one
below, at and one above, and a frame smaller than a tile), 256 x 144, and the special inputs.  EQUIVALENCE of the host-pointer and device
routes, of a second filter and a fresh handle, of reset + load.  RENDERED frames (a Progress handle's frame and stderr, albedo from
render_aov): bit for bit, and closer to a 8192-spp reference than the noisy frame.  Refusals that need a handle, non-interference with
vk_render, a live progress handle, vk_denoise and a tone handle, and the live-object count."""
import ctypes as C

import numpy as np
import pytest

import emu_nlm_ffi as EMU
import nlm_ref as R
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMS = (ffi.VK_NLM_FORM_PLAIN, ffi.VK_NLM_FORM_TILED, ffi.VK_NLM_FORM_AUTO)
RADII = [(r, f) for r in (1, 3, 10) for f in (0, 1, 3)]
SIZES = [(1, 1), (1, 7), (7, 1), (5, 5), (33, 9), (65, 17), (31, 7), (32, 8), (63, 5), (64, 3)]


@pytest.fixture(scope="module")
def scene(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    yield ds
    ds.close()


def all_forms(nl, want, want_se, what, **kw):
    for form in FORMS:
        nl.set_form(form)
        got, got_se = nl.filter(**kw)
        assert R.same_bits(got, want), (what, form, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4].tolist())
        assert R.same_bits(got_se, want_se), (what, form, np.argwhere(got_se.view(np.uint32) != want_se.view(np.uint32))[:4].tolist())
        # AUTO's table (DESIGN.md "Non-local means"): the plain form without a patch, the tiled form with one
        auto = ffi.VK_NLM_FORM_PLAIN if kw.get("patch_radius", 3) == 0 else ffi.VK_NLM_FORM_TILED
        assert nl.info().last_form == (form or auto), (what, form)


# ---------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_device_equals_the_restatement_and_the_host_build(size, scene, emu):
    W, H = size
    color, se, albedo = R.synthetic(W, H, seed=100 * W + H)
    with scene.nlm(W, H) as nl:
        for alb in (albedo, None):
            nl.load(color, se, alb)
            assert nl.info().has_albedo == (alb is not None)
            for r, f in RADII:
                want, want_se = R.filter(color, se, alb, r, f)
                emu_out, emu_se = EMU.filter(color, se, alb, r, f)
                assert R.same_bits(emu_out, want) and R.same_bits(emu_se, want_se)
                all_forms(nl, want, want_se, (size, r, f, alb is None), search_radius=r, patch_radius=f)
            only, none = nl.filter(search_radius=3, patch_radius=1, want_stderr=False)
            assert none is None and R.same_bits(only, R.filter(color, se, alb, 3, 1)[0])
        # (both kernels have been timed; how long a kernel over so few pixels takes is not asserted: test_256x144 holds the times)
        ms = nl.last_ms()
        assert all(np.isfinite(m) and m >= 0 for m in ms) and nl.info().last_kernel_ms == ms[1]


@pytest.mark.parametrize("radii", RADII, ids=[f"R{r}F{f}" for r, f in RADII])
def test_256x144(radii, scene):
    r, f = radii
    W, H = 256, 144
    color, se, albedo = R.synthetic(W, H, seed=77)
    color[70:80, 100:111] = np.nan
    want, want_se = R.filter(color, se, albedo, r, f)
    with scene.nlm(W, H) as nl:
        nl.load(color, se, albedo)
        all_forms(nl, want, want_se, radii, search_radius=r, patch_radius=f)
        nl.set_form(ffi.VK_NLM_FORM_PLAIN)
        nl.filter(search_radius=r, patch_radius=f)
        # 36 864 pixels, 9 to 441 offsets each: tens of microseconds at the least, far above the events' resolution
        assert min(nl.last_ms()) > 0 and nl.info().last_kernel_ms == nl.last_ms()[1] and nl.info().last_form == ffi.VK_NLM_FORM_PLAIN


@pytest.mark.parametrize("size", [(33, 9), (65, 17)], ids=["33x9", "65x17"])
def test_special_inputs(size, scene):
    W, H = size
    with scene.nlm(W, H) as nl:
        for name, (color, se, albedo) in R.special_cases(W, H, seed=3).items():
            nl.load(color, se, albedo)
            for r, f in ((3, 1), (10, 3)):
                want, want_se = R.filter(color, se, albedo, r, f)
                all_forms(nl, want, want_se, (size, name, r, f), search_radius=r, patch_radius=f)


def test_other_parameters_and_the_floor(scene):
    W, H = 65, 17
    color, se, albedo = R.special_cases(W, H, seed=4)["albedo_zero"]
    with scene.nlm(W, H) as nl:
        nl.load(color, se, albedo)
        for kw in (dict(k=0.9, alpha=0.25), dict(k=0.3, alpha=0.0), dict(albedo_floor=0.5), dict(albedo_floor=1e-3, k=2.0)):
            want, want_se = R.filter(color, se, albedo, 3, 1, kw.get("k", 0.45), kw.get("alpha", 1.0), kw.get("albedo_floor", 1e-3))
            all_forms(nl, want, want_se, kw, search_radius=3, patch_radius=1, **kw)
        assert nl.info().loads == 1                   # another floor prepares again from the handle's copy: no reload


# ---------------------------------------------------------------- 2. equivalence
def test_routes_second_filter_and_reset(scene):
    import torch
    W, H = 65, 17
    color, se, albedo = R.synthetic(W, H, seed=21)
    other, other_se, _ = R.synthetic(W, H, seed=22)
    with scene.nlm(W, H) as a, scene.nlm(W, H) as b:
        a.load(color, se, albedo)
        first = a.filter(search_radius=3, patch_radius=1)
        second = a.filter(search_radius=7, patch_radius=3, k=0.7)               # a second filter, other parameters, no reload
        b.load(color, se, albedo)
        fresh = b.filter(search_radius=7, patch_radius=3, k=0.7)
        assert R.same_bits(second[0], fresh[0]) and R.same_bits(second[1], fresh[1]) and a.info().loads == 1 and a.info().filters == 2
        # the device route
        d = [torch.from_numpy(x).cuda() for x in (color, se, albedo)]
        b.load_device(*d)
        for t in d:
            t.zero_()                                                            # the caller's buffers may be reused after the load
        d_out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
        d_se = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
        b.filter_device(d_out, d_se, search_radius=3, patch_radius=1)
        assert b.last_ms()[1] >= 0                                               # (waits for the event behind the filter)
        torch.cuda.synchronize()
        assert R.same_bits(d_out.cpu().numpy(), first[0]) and R.same_bits(d_se.cpu().numpy(), first[1])
        d_only = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
        b.filter_device(d_only.data_ptr(), None, search_radius=3, patch_radius=1)       # a bare pointer, no stderr3_out
        torch.cuda.synchronize()
        assert R.same_bits(d_only.cpu().numpy(), first[0])
        # reset, then another frame without albedo
        a.reset()
        assert a.info().loaded == 0
        a.load(other, other_se)
        want = R.filter(other, other_se, None, 3, 1)
        got = a.filter(search_radius=3, patch_radius=1)
        assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1]) and a.info().has_albedo == 0


# ---------------------------------------------------------------- 3. rendered inputs
# The ratio relMSE(nlm) / relMSE(noisy) of each frame as tests/nlm_ref.py — the restatement, not the library — gives it at the shipped
# defaults, measured once on the frames this test renders (DESIGN.md "Non-local means"); the device's frame, which equals the
# restatement's bit for bit, must keep at least half of that improvement: the project's margin for a seed-dependent figure.
R_MEASURED = {"cornell_box": 0.0253,             # 128 x 128: relMSE 0.43032 -> 0.01087
              "random_spheres_iow": 0.5599}      # 256 x 144: relMSE 0.01047 -> 0.00586


def rendered(ds, hs, cam, width, height, spp=16, windows=4):
    p = hs.params(width, spp, 50, seed=5, height=height)
    with ds.progress(cam, p, stderr=True) as pr:
        for _ in range(windows):
            img, _ = pr.step(spp // windows)
        se = pr.stderr()
    aov, _ = ds.render_aov(cam, p)
    return img.copy(), se, aov["albedo"]


@pytest.mark.parametrize("name,width,height", [("cornell_box", 128, 128), ("random_spheres_iow", 256, 144)])
def test_rendered_frames(name, width, height, device, host_scenes):
    hs, cam = host_scenes(name)
    ds = DeviceScene(hs.desc)
    try:
        color, se, albedo = rendered(ds, hs, cam, width, height)
        truth, _ = ds.render(cam, hs.params(width, 8192, 50, seed=77, height=height))
        want, want_se = R.filter(color, se, albedo)
        with ds.nlm(width, height) as nl:
            nl.load(color, se, albedo)
            all_forms(nl, want, want_se, name)
            got, _ = nl.filter()
        noisy, clean = R.rel_mse(color, truth), R.rel_mse(got, truth)
        print(f"{name}: relMSE noisy {noisy:.5f} nlm {clean:.5f} ratio {clean / noisy:.4f} (restatement {R.rel_mse(want, truth) / noisy:.4f})")
        assert clean < noisy
        assert clean / noisy <= 1 - (1 - R_MEASURED[name]) / 2, (clean / noisy, R_MEASURED[name])
    finally:
        ds.close()


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
        W, H = 9, 5
        nl = ds.nlm(W, H)
        assert live()[0] == before[0] + 2 and live()[2] == before[2] + 4
        color, se, albedo = R.synthetic(W, H, seed=2)
        out, out_se = np.full((H, W, 3), 7, f32), np.full((H, W, 3), 7, f32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)

        def refused(p, word):
            assert dbg.vk_nlm_filter(nl._h, C.byref(p), ptr(out), ptr(out_se)) == ffi.VK_ERR_BAD_ARG and word in dbg.vk_last_error(), word
            assert (out == 7).all() and (out_se == 7).all()

        refused(nl.params(), b"vk_nlm_filter before vk_nlm_load")
        assert dbg.vk_nlm_load(nl._h, ptr(color), None, None) == ffi.VK_ERR_BAD_ARG and dbg.vk_nlm_load(nl._h, None, ptr(se), None) == ffi.VK_ERR_BAD_ARG
        assert nl.info().loaded == 0 and nl.info().loads == 0
        nl.load(color, se, albedo)
        refused(nl.params(search_radius=0), b"search_radius must be in 1..10")
        refused(nl.params(search_radius=11), b"search_radius must be in 1..10")
        refused(nl.params(patch_radius=4), b"patch_radius must be in 0..3")
        refused(nl.params(flags=1), b"unknown nlm flags")
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(nl.params(k=bad), b"k must be finite and > 0")
            refused(nl.params(albedo_floor=bad), b"albedo_floor must be finite and > 0")
        for bad in (-1.0, float("nan"), float("inf")):
            refused(nl.params(alpha=bad), b"alpha must be finite and >= 0")
        assert dbg.vk_nlm_filter(nl._h, C.byref(nl.params()), None, ptr(out_se)) == ffi.VK_ERR_BAD_ARG and (out_se == 7).all()
        assert nl.info().filters == 0
        assert nl.filter(alpha=0.0)[0].shape == (H, W, 3)                      # alpha = 0 is admitted
        assert live()[0] == before[0] + 3                                        # the outputs' buffer, on the first host filter
        assert nl.info().scratch_bytes == W * H * 4 * (9 + 12 + 6)
        nl.reset()
        refused(nl.params(), b"vk_nlm_filter before vk_nlm_load")             # reset forgets the frame
        assert dbg.vk_debug_nlm_set_form(nl._h, 3) == ffi.VK_ERR_BAD_ARG and b"unknown nlm form" in dbg.vk_last_error()
        nl.close()
        assert live() == before
        dbg.vk_nlm_destroy(None)
    finally:
        ds.close()


# ---------------------------------------------------------------- 5. non-interference
def test_leaves_renders_progress_denoise_and_tone_alone(scene, host_scenes):
    hs, cam = host_scenes("cornell_box")
    ds = scene
    p = hs.params(32, 16, 12, seed=4)
    color, se, albedo = R.synthetic(48, 40, seed=9)
    launches = lambda: [bytes(x) for x in ffi.last_launches(ds._lib, ds._h)]
    aov, _ = ds.render_aov(cam, hs.params(48, 4, 12, seed=4, height=40))
    a, sa = ds.render(cam, p)
    la, ra, ms = launches(), ds.last_requeued_samples(), ds.last_kernel_ms()
    dn_before, _ = ds.denoise(color, se, albedo, aov["normal"], aov["depth"])
    with ds.nlm(48, 40) as nl:                                                   # vk_render's figures, before anything else renders
        nl.load(color, se, albedo)
        nl.filter(search_radius=3, patch_radius=1)
        assert launches() == la and ds.last_requeued_samples() == ra and ds.last_kernel_ms() == ms
    with ds.tone(32, 32) as t, ds.progress(cam, p) as pr, ds.nlm(48, 40) as nl:
        t.load(a)
        info = t.meter()
        codes = t.encode()
        hist = t.histogram()[0]
        pr.step(6)
        nl.load(color, se, albedo)                                               # between two steps of a live progress handle
        for form in FORMS:
            nl.set_form(form)
            nl.filter(search_radius=3, patch_radius=1)
        img, _ = pr.step(10)
        assert R.same_bits(img, a)
        assert np.array_equal(t.encode(), codes) and t.info().exposure == info.exposure and np.array_equal(t.histogram()[0], hist)
    a, sa = ds.render(cam, p)
    la = launches()
    with ds.nlm(48, 40) as nl:
        nl.load(color, se, albedo)
        nl.filter()
    b, sb = ds.render(cam, p)
    assert R.same_bits(b, a) and launches() == la and sb.clamped_samples == sa.clamped_samples
    dn_after, _ = ds.denoise(color, se, albedo, aov["normal"], aov["depth"])
    assert R.same_bits(dn_after, dn_before)
