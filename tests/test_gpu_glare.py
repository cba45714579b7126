"""-m gpu: glare (vk_glare_*) on the MI355X.  RESTATEMENT: the device's frame equals tests/glare_ref.py and the host build of vk_glare.h
bit for bit (a NaN's payload aside) in the PLAIN, FUSED and AUTO forms — the CPU test's sizes, 256 x 144, and 317 x 301 and 321 x 311,
which lie on either side of the tail's limit (level 2 of the first, 80 x 76, fits the tail's 6144 floats; of the second, 81 x 78, does
not) and end the LDS kernels' tiles (32 x 8 and 16 x 8) part-way.  EQUIVALENCE of the host-pointer and device routes, in place, a second
apply with other parameters.  LAUNCHES: the plan's counts, FUSED below PLAIN from L = 3 on; AUTO's rule.  A RENDERED Cornell frame
through glare and the display transform; the command-line tool's glare argument.  Refusals on a live handle, non-interference with
vk_render, and the live-object count."""
import ctypes as C

import numpy as np
import pytest

import emu_glare_ffi as EMU
import glare_ref as R
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMS = (ffi.VK_GLARE_FORM_PLAIN, ffi.VK_GLARE_FORM_FUSED, ffi.VK_GLARE_FORM_AUTO)
SIZES = [(1, 1), (2, 3), (5, 1), (37, 53), (64, 32), (130, 70), (256, 144), (317, 301), (321, 311)]
CASES = [(L, 0.3, fo, th) for L in (1, 2, 3, 4, 6, 8) for fo, th in ((1.0, 0.0), (0.5, 1.0))] + [(6, 1.0, 2.0, 0.0), (5, 0.0, 1.0, 0.25)]


def auto_form(W, H, L):
    """AUTO's documented rule (DESIGN.md "Glare"), a function of the size and L only: the plain form everywhere — the fused form was
    measured faster at no size"""
    return ffi.VK_GLARE_FORM_PLAIN


@pytest.fixture(scope="module")
def scene(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    yield ds
    ds.close()


def differing(a, b):
    return np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:4].tolist()


# ---------------------------------------------------------------- 1. the restatement, the launch plan and AUTO's rule
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_device_equals_the_restatement_and_the_host_build(size, scene, emu):
    W, H = size
    I = R.hdr_frame(W, H, seed=100 * W + H)
    with scene.glare(W, H) as g:
        for L, st, fo, th in CASES:
            want = R.apply(I, L, st, fo, th)
            assert R.same_bits(EMU.apply(I, L, st, fo, th), want)
            for form in FORMS:
                g.set_form(form)
                got = g.apply(I, levels=L, strength=st, falloff=fo, threshold=th)
                assert R.same_bits(got, want), (size, L, st, fo, th, form, differing(got, want))
                info = g.info()
                used = form or auto_form(W, H, L)
                assert info.last_form == used and info.last_levels == L, (size, L, form)
                assert info.last_launches == EMU.launch_count(W, H, L, used), (size, L, form, info.last_launches)
                if form == ffi.VK_GLARE_FORM_PLAIN:
                    assert info.last_launches == max(1, 2 * L - 2)
                elif form == ffi.VK_GLARE_FORM_FUSED and L >= 3:
                    assert info.last_launches < 2 * L - 2
        ms = g.last_ms()
        assert np.isfinite(ms) and ms >= 0 and g.info().last_kernel_ms == ms and g.info().applies == 3 * len(CASES)


# Frames whose tail starts at level 3 and at level 4, as the report frames' do: FUSED then runs the two-level kernel, the LDS down pass
# from a stored plane (B_2 -> B_3, and B_3 -> B_4) and plain up passes behind the tail.  Sizes that end every tile part-way.
LARGE = [((641, 637), 3), ((1283, 1279), 4)]
LARGE_CASES = [(4, 0.3, 1.0, 0.0), (5, 0.3, 0.5, 1.0), (6, 0.15, 1.0, 0.0), (8, 0.3, 2.0, 0.0)]


@pytest.mark.parametrize("size,tail", LARGE, ids=[f"{s[0]}x{s[1]}" for s, _ in LARGE])
def test_large_frames_with_a_late_tail(size, tail, scene, emu):
    W, H = size
    assert EMU.tail_level(W, H) == tail
    I = R.hdr_frame(W, H, seed=100 * W + H)
    with scene.glare(W, H) as g:
        for L, st, fo, th in LARGE_CASES:
            want = R.apply(I, L, st, fo, th)
            for form in FORMS:
                g.set_form(form)
                got = g.apply(I, levels=L, strength=st, falloff=fo, threshold=th)
                assert R.same_bits(got, want), (size, L, st, fo, th, form, differing(got, want))
                used = form or auto_form(W, H, L)
                assert g.info().last_form == used and g.info().last_launches == EMU.launch_count(W, H, L, used)
            # the fused plan: B_1 and B_2 in one launch, LDS down passes up to B_min(t, L - 1), the tail if it has levels to make, the up
            # passes below it, the composite
            m = tail if tail + 2 <= L else L - 1
            assert EMU.launch_count(W, H, L, ffi.VK_GLARE_FORM_FUSED) == (m - 1) + (1 if tail + 2 <= L else 0) + (m - 1) + 1 < 2 * L - 2


# ---------------------------------------------------------------- 2. routes, in place, a second apply
def test_routes_in_place_and_a_second_apply(scene):
    import torch
    W, H = 130, 70
    I = R.hdr_frame(W, H, seed=11)
    first, second = R.apply(I, 6, 0.15, 1.0, 0.0), R.apply(I, 3, 0.9, 0.5, 2.0)
    with scene.glare(W, H) as g:
        for form in FORMS:
            g.set_form(form)
            assert R.same_bits(g.apply(I), first)                                   # the defaults: levels 6, strength 0.15
            d_in = torch.from_numpy(I).cuda()
            d_out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
            assert g.apply_device(d_in, d_out) is d_out
            assert g.last_ms() >= 0                                                 # (waits for the event behind the composite)
            torch.cuda.synchronize()
            assert R.same_bits(d_out.cpu().numpy(), first) and R.same_bits(d_in.cpu().numpy(), I)
            g.apply_device(d_in.data_ptr(), d_out.data_ptr(), levels=3, strength=0.9, falloff=0.5, threshold=2.0)      # bare pointers, other parameters
            torch.cuda.synchronize()
            assert R.same_bits(d_out.cpu().numpy(), second)
            g.apply_device(d_in, levels=3, strength=0.9, falloff=0.5, threshold=2.0)                                    # in place
            torch.cuda.synchronize()
            assert R.same_bits(d_in.cpu().numpy(), second), form
            again = I.copy()
            p = g.params()
            assert g._lib.vk_glare_apply(g._h, C.byref(p), C.c_void_p(again.ctypes.data), C.c_void_p(again.ctypes.data)) == ffi.VK_OK
            assert R.same_bits(again, first)                                        # the host-pointer route in place


# ---------------------------------------------------------------- 3. a rendered frame through glare and the display transform
def test_rendered_cornell_through_glare_and_tone(scene, host_scenes):
    import torch
    hs, cam = host_scenes("cornell_box")
    frame, _ = scene.render(cam, hs.params(64, 16, 12, seed=3, height=64))
    frame = np.ascontiguousarray(frame, f32).reshape(64, 64, 3)
    want = R.apply(frame)
    assert not R.same_bits(want, frame)
    with scene.glare(64, 64) as g, scene.tone(64, 64) as t:
        t.load(want)
        t.meter()
        codes_want = t.encode()
        d = torch.from_numpy(frame).cuda()
        g.apply_device(d)
        t.load_device(d)
        t.meter()
        codes = t.encode()
        torch.cuda.synchronize()
        assert R.same_bits(d.cpu().numpy(), want)
        assert np.array_equal(codes, codes_want)


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
        g = ds.glare(W, H)
        assert live()[0] == before[0] + 1 and live()[2] == before[2] + 2             # the pyramid; two events
        planes = sum(w * h for w, h in R.sizes(W, H, 8)[1:])
        assert g.info().scratch_bytes == 2 * planes * 12 and g.info().applies == 0 and g.info().last_form == 0
        I = R.hdr_frame(W, H, seed=2)
        out = np.full((H, W, 3), 7, f32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)

        def refused(p, word):
            assert dbg.vk_glare_apply(g._h, C.byref(p), ptr(I), ptr(out)) == ffi.VK_ERR_BAD_ARG and word in dbg.vk_last_error(), word
            assert (out == 7).all()

        refused(g.params(levels=0), b"levels must be in 1..8")
        refused(g.params(levels=9), b"levels must be in 1..8")
        refused(g.params(flags=1), b"unknown glare flags")
        refused(g.params(_pad=2), b"unknown glare flags")
        for bad in (-0.5, 1.5, float("nan"), float("inf")):
            refused(g.params(strength=bad), b"strength must be in [0, 1]")
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(g.params(falloff=bad), b"falloff must be finite and > 0")
        for bad in (-1.0, float("nan"), float("inf")):
            refused(g.params(threshold=bad), b"threshold must be finite and >= 0")
        ok = g.params()
        assert dbg.vk_glare_apply(g._h, C.byref(ok), None, ptr(out)) == ffi.VK_ERR_BAD_ARG and (out == 7).all()
        assert dbg.vk_glare_apply(g._h, C.byref(ok), ptr(I), None) == ffi.VK_ERR_BAD_ARG
        assert dbg.vk_glare_apply_device(g._h, C.byref(ok), None, ptr(out)) == ffi.VK_ERR_BAD_ARG
        assert g.info().applies == 0 and live()[0] == before[0] + 1
        assert R.same_bits(g.apply(I, strength=1.0, levels=8), R.apply(I, 8, 1.0))    # strength 1 and levels 8 are admitted
        assert live()[0] == before[0] + 2                                             # the frames in and out, on the first host apply
        assert g.info().scratch_bytes == 2 * planes * 12 + 2 * W * H * 12 and g.info().applies == 1
        assert dbg.vk_debug_glare_set_form(g._h, 3) == ffi.VK_ERR_BAD_ARG and b"unknown glare form" in dbg.vk_last_error()
        g.close()
        assert live() == before
        dbg.vk_glare_destroy(None)
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
    I = R.hdr_frame(48, 40, seed=9)
    with ds.glare(48, 40) as g:
        for form in FORMS:
            g.set_form(form)
            g.apply(I)
        assert launches() == la and ds.last_requeued_samples() == ra and ds.last_kernel_ms() == ms
    b, sb = ds.render(cam, p)
    assert R.same_bits(b, a) and launches() == la and sb.clamped_samples == sa.clamped_samples


# ---------------------------------------------------------------- 6. the command-line tool's glare argument
def test_cli_glare_argument(device, host_scenes, tmp_path):
    import subprocess
    from test_gpu_aov import _read_pfm
    from test_gpu_tone import read_ppm
    from vecchio_amd import build
    cli = build.build_cli()
    # (aov_spp = 1 writes the float frame, output_0000.pfm; display = 3: ACES)
    base = ["cornell_box", "64", "16", "20", "1", "1", "1", "1", "0", "0", "0", "3"]
    dirs = {}
    for key, extra in (("absent", []), ("glare", ["40"])):
        dirs[key] = tmp_path / key
        dirs[key].mkdir()
        subprocess.run([cli] + base + extra, cwd=dirs[key], check=True, timeout=300, capture_output=True)
    names = sorted(f.name for f in dirs["absent"].iterdir())
    assert sorted(f.name for f in dirs["glare"].iterdir()) == sorted(names + ["output_0000_glare.pfm"])
    for n in names:
        if n != "output_0000_display.ppm":
            assert (dirs["absent"] / n).read_bytes() == (dirs["glare"] / n).read_bytes(), n
    frame = _read_pfm(dirs["glare"] / "output_0000.pfm")
    want = R.apply(frame, 6, f32(40) / f32(100), 1.0, 0.0)
    assert R.same_bits(_read_pfm(dirs["glare"] / "output_0000_glare.pfm"), want)
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    try:
        with ds.tone(64, 64) as t:
            t.load(want)
            t.meter()
            codes = t.encode()
        assert np.array_equal(read_ppm(dirs["glare"] / "output_0000_display.ppm"), codes.astype(np.int64))
        assert not np.array_equal(read_ppm(dirs["absent"] / "output_0000_display.ppm"), codes.astype(np.int64))
    finally:
        ds.close()
