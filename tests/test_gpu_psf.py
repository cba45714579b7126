"""-m gpu: the point-spread stage (vk_psf_*) on the MI355X.  RESTATEMENT: the device's frame equals the host build of vk_psf.h (every
case of tests/psf_cases.py) and tests/psf_ref.py (a subset) as floats in the PLAIN, LDS and AUTO forms; the bare transform
vk_psf_debug_fft2 forward and inverse against the restatement.  A RELOAD with another K under one handle; EQUIVALENCE of the host-pointer
and device routes, in place, a second apply with other parameters.  AUTO's rule and the launch counts.  A RENDERED Cornell frame through
glare, the point-spread stage and the display transform.  Refusals on a live handle, non-interference with a glare and a tone handle and
with vk_render, and the live-object count."""
import ctypes as C

import numpy as np
import pytest

import emu_psf_ffi as EMU
import psf_cases as PC
import psf_ref as R
from vecchio_amd import DeviceScene, ffi
from vecchio_amd.scene import Psf

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMS = (ffi.VK_PSF_FORM_PLAIN, ffi.VK_PSF_FORM_LDS, ffi.VK_PSF_FORM_AUTO)
NAMES = [c[0] for c in PC.CASES]


def auto_form(W, H, K):
    """AUTO's documented rule (DESIGN.md "Point-spread function"): the LDS form everywhere"""
    return ffi.VK_PSF_FORM_LDS


def plain_launches(Px, Py):
    """pad; per transform a bit reversal and the stages of each axis; the product; the composite"""
    mx, my = Px.bit_length() - 1, Py.bit_length() - 1
    return 1 + 2 * ((1 + mx) + (1 + my)) + 1 + 1


@pytest.fixture(scope="module")
def scene(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    yield ds
    ds.close()


def differing(a, b):
    return np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))[:4].tolist()


# ---------------------------------------------------------------- 1. the restatement, the launch counts and AUTO's rule
@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_host_build_and_the_restatement(name, scene, emu):
    _, W, H, K, st, th, _, _ = PC.case(name)
    I, k, _, _ = PC.inputs(name)
    want = EMU.apply(I, k, st, th)
    if name in PC.SUBSET:
        assert R.same_floats(R.apply(I, k, st, th), want)
    Px, Py = R.padded(W, H, K)
    with scene.psf(W, H, K) as g:
        g.load(k)
        info = g.info()
        assert (info.K, info.Px, info.Py, info.loads, info.applies, info.last_form) == (K, Px, Py, 1, 0, 0)
        for form in FORMS:
            got = g.apply(I, strength=st, threshold=th, form=form)
            assert R.same_floats(got, want), (name, form, differing(got, want))
            info = g.info()
            used = form or auto_form(W, H, K)
            assert info.last_form == used, (name, form)
            assert info.last_launches == (plain_launches(Px, Py) if used == ffi.VK_PSF_FORM_PLAIN else 4), (name, form, info.last_launches)
            passes = g.last_pass_ms()
            assert len(passes) == 4 and all(np.isfinite(p) and p >= 0 for p in passes)
            assert (used == ffi.VK_PSF_FORM_LDS or sum(passes) == 0) and sum(passes) <= info.last_kernel_ms * 1.01 + 1e-3
        assert g.info().applies == 3 and np.isfinite(g.info().last_kernel_ms) and g.info().last_kernel_ms >= 0
        if st == 0.0:
            assert R.same_floats(want, I)


FFT_SIZES = [(2, 2), (4, 2), (2, 8), (64, 16), (128, 512), (4096, 4), (4, 4096), (512, 256)]


@pytest.mark.parametrize("size", FFT_SIZES, ids=[f"{x}x{y}" for x, y in FFT_SIZES])
def test_the_bare_transform_forward_then_inverse(size, scene, emu):
    """vk_psf_debug_fft2 in both forms against the restatement and the host build: forward, then the inverse of that (which brings the
    input back within rounding)"""
    Px, Py = size
    rng = np.random.default_rng(Px * 7 + Py)
    a = rng.normal(0, 1, (Py, Px, 2)).astype(f32)
    fr, fi = R.fft2(a[..., 0], a[..., 1])
    fwd = np.stack([fr, fi], axis=-1)
    br, bi = R.fft2(fr, fi, inverse=True)
    back = np.stack([br, bi], axis=-1)
    assert R.same_floats(EMU.fft2(a), fwd) and R.same_floats(EMU.fft2(fwd, inverse=True), back)
    import psf_laws_ref
    assert np.abs(back.astype(np.float64) - a).max() <= psf_laws_ref.roundtrip_bound(Px, Py, a)
    lib = scene._lib
    for form in (ffi.VK_PSF_FORM_PLAIN, ffi.VK_PSF_FORM_LDS):
        d = a.copy()
        assert lib.vk_psf_debug_fft2(scene._h, Px, Py, 0, form, C.c_void_p(d.ctypes.data)) == ffi.VK_OK, lib.vk_last_error()
        assert R.same_floats(d, fwd), (size, form, differing(d, fwd))
        assert lib.vk_psf_debug_fft2(scene._h, Px, Py, 1, form, C.c_void_p(d.ctypes.data)) == ffi.VK_OK
        assert R.same_floats(d, back), (size, form, differing(d, back))


def test_the_librarys_twiddle_tables(scene):
    lib = scene._lib
    for N in (2, 4, 64, 4096):
        T = np.zeros((N // 2, 2), f32)
        assert lib.vk_psf_debug_twiddles(N, C.c_void_p(T.ctypes.data)) == ffi.VK_OK
        assert np.array_equal(T.view(np.uint32), R.twiddles(N).view(np.uint32)), N


# ---------------------------------------------------------------- 2. a reload, routes, in place, a second apply
def test_reload_routes_in_place_and_a_second_apply(scene, emu):
    import torch
    W, H = 61, 7
    I = PC.frame(W, H, 21, True)
    k5, k9 = PC.kernel(5, 21), PC.kernel(9, 22)
    first, second = EMU.apply(I, k5, 0.15, 0.0), EMU.apply(I, k9, 0.9, 2.0)
    with scene.psf(W, H, 9) as g:
        for form in FORMS:
            g.load(k5)
            assert (g.info().K, g.info().Px, g.info().Py) == (5, 128, 16)
            assert R.same_floats(g.apply(I, form=form), first)                       # the defaults: strength 0.15, threshold 0
            d_in = torch.from_numpy(I).cuda()
            d_out = torch.full((H, W, 3), 7.0, dtype=torch.float32, device="cuda")
            assert g.apply_device(d_in, d_out, form=form) is d_out
            assert g.info().last_kernel_ms >= 0                                     # (waits for the event behind the last kernel)
            torch.cuda.synchronize()
            assert R.same_floats(d_out.cpu().numpy(), first) and R.same_floats(d_in.cpu().numpy(), I)
            g.load_device(9, torch.from_numpy(k9).cuda())                           # another K under the same handle, from the device
            assert (g.info().K, g.info().Px, g.info().Py) == (9, 128, 16)
            g.apply_device(d_in.data_ptr(), d_out.data_ptr(), strength=0.9, threshold=2.0, form=form)      # bare pointers, other parameters
            torch.cuda.synchronize()
            assert R.same_floats(d_out.cpu().numpy(), second)
            g.apply_device(d_in, strength=0.9, threshold=2.0, form=form)           # in place
            torch.cuda.synchronize()
            assert R.same_floats(d_in.cpu().numpy(), second), form
            again = I.copy()
            p = g.params(strength=0.9, threshold=2.0, form=form)
            assert g._lib.vk_psf_apply(g._h, C.byref(p), C.c_void_p(again.ctypes.data), C.c_void_p(again.ctypes.data)) == ffi.VK_OK
            assert R.same_floats(again, second)                                     # the host-pointer route in place
        assert g.info().loads == 6 and g.info().applies == 15


# ---------------------------------------------------------------- 3. a rendered frame through glare, the star and the display transform
def test_rendered_cornell_through_glare_psf_and_tone(scene, host_scenes, emu):
    import torch
    import glare_ref
    hs, cam = host_scenes("cornell_box")
    frame, _ = scene.render(cam, hs.params(64, 16, 12, seed=3, height=64))
    frame = np.ascontiguousarray(frame, f32).reshape(64, 64, 3)
    star = Psf.star(31, streaks=6, chroma=0.1, lib=scene._lib)
    glared = glare_ref.apply(frame)
    want = EMU.apply(glared, star, 0.15, 0.0)
    assert not R.same_floats(want, glared)
    with scene.glare(64, 64) as gl, scene.psf(64, 64, 31) as g, scene.tone(64, 64) as t:
        g.load(star)
        t.load(want)
        t.meter()
        codes_want = t.encode()
        d = torch.from_numpy(frame).cuda()
        gl.apply_device(d)
        g.apply_device(d)
        t.load_device(d)
        t.meter()
        codes = t.encode()
        torch.cuda.synchronize()
        assert R.same_floats(d.cpu().numpy(), want)
        assert np.array_equal(codes, codes_want)


# ---------------------------------------------------------------- 4. refusals that need a handle, and what a handle owns
def test_refusals_with_a_handle_and_live_objects(device, host_scenes, emu):
    dbg = ffi.load_debug_lib()
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc, lib=dbg)

    def live():
        out = (C.c_uint64 * 4)()
        assert dbg.vk_debug_live_objects(C.byref(out)) == ffi.VK_OK
        return tuple(out)

    try:
        before = live()
        W, H, kmax = 9, 5, 7
        g = ds.psf(W, H, kmax)
        assert live()[0] == before[0] + 4 and live()[2] == before[2] + 5             # F, G, the tables, the kernel; five events
        Px, Py = R.padded(W, H, kmax)
        owned = 2 * 3 * Px * Py * 8 + (Px // 2 + Py // 2) * 8 + kmax * kmax * 12
        assert g.info().scratch_bytes == owned and g.info().applies == 0 and g.info().last_form == 0 and g.info().kmax == kmax
        I = PC.frame(W, H, 2, True)
        out = np.full((H, W, 3), 7, f32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)
        ok = g.params()
        # apply before a load
        assert dbg.vk_psf_apply(g._h, C.byref(ok), ptr(I), ptr(out)) == ffi.VK_ERR_BAD_ARG and b"before vk_psf_load" in dbg.vk_last_error()
        # loads that are refused leave the handle without a kernel
        k = PC.kernel(5, 3)
        for K, word in ((4, b"K must be odd"), (1, b"K must be odd"), (1025, b"K must be odd"), (9, b"exceeds the handle's kmax")):
            assert dbg.vk_psf_load(g._h, K, ptr(k)) == ffi.VK_ERR_BAD_ARG and word in dbg.vk_last_error(), K
        assert dbg.vk_psf_load(g._h, 5, None) == ffi.VK_ERR_BAD_ARG
        for bad, word in ((np.nan, b"not finite"), (np.inf, b"not finite"), (-1e-9, b"negative")):
            kb = k.copy()
            kb[3, 1, 2] = bad
            assert dbg.vk_psf_load(g._h, 5, ptr(kb)) == ffi.VK_ERR_BAD_ARG and word in dbg.vk_last_error(), bad
        kb = k.copy()
        kb[..., 1] = 0
        assert dbg.vk_psf_load(g._h, 5, ptr(kb)) == ffi.VK_ERR_BAD_ARG and b"sums to nothing" in dbg.vk_last_error()
        assert g.info().K == 0 and g.info().loads == 0
        g.load(k)

        def refused(p, word):
            assert dbg.vk_psf_apply(g._h, C.byref(p), ptr(I), ptr(out)) == ffi.VK_ERR_BAD_ARG and word in dbg.vk_last_error(), word
            assert (out == 7).all()

        refused(g.params(form=3), b"unknown psf form")
        refused(g.params(flags=1), b"unknown psf flags")
        refused(g.params(_pad=2), b"unknown psf flags")
        for bad in (-0.5, 1.5, float("nan"), float("inf")):
            refused(g.params(strength=bad), b"strength must be in [0, 1]")
        for bad in (-1.0, float("nan"), float("inf")):
            refused(g.params(threshold=bad), b"threshold must be finite and >= 0")
        assert dbg.vk_psf_apply(g._h, C.byref(ok), None, ptr(out)) == ffi.VK_ERR_BAD_ARG and (out == 7).all()
        assert dbg.vk_psf_apply(g._h, C.byref(ok), ptr(I), None) == ffi.VK_ERR_BAD_ARG
        assert dbg.vk_psf_apply_device(g._h, C.byref(ok), None, ptr(out)) == ffi.VK_ERR_BAD_ARG
        assert g.info().applies == 0 and live()[0] == before[0] + 4
        assert R.same_floats(g.apply(I, strength=1.0), EMU.apply(I, k, 1.0, 0.0))      # strength 1 is admitted
        assert live()[0] == before[0] + 5                                             # the frames in and out, on the first host apply
        assert g.info().scratch_bytes == owned + 2 * W * H * 12 and g.info().applies == 1
        g.reset()
        assert g.info().K == 0
        assert dbg.vk_psf_apply(g._h, C.byref(ok), ptr(I), ptr(out)) == ffi.VK_ERR_BAD_ARG and (out == 7).all()
        g.close()
        assert live() == before
        dbg.vk_psf_destroy(None)
        # sizes create refuses
        h = C.c_void_p(0x77)
        for dims in ((4096, 4, 3), (4, 4095, 3), (3075, 8, 1023)):
            assert dbg.vk_psf_create(ds._h, *dims, C.byref(h)) == ffi.VK_ERR_BAD_ARG and b"exceeds 4096" in dbg.vk_last_error(), dims
        assert h.value == 0x77
    finally:
        ds.close()


# ---------------------------------------------------------------- 5. non-interference
def test_leaves_renders_glare_and_tone_alone(scene, host_scenes):
    import glare_ref
    hs, cam = host_scenes("cornell_box")
    ds = scene
    p = hs.params(32, 16, 12, seed=4)
    launches = lambda: [bytes(x) for x in ffi.last_launches(ds._lib, ds._h)]
    a, sa = ds.render(cam, p)
    la, ra, ms = launches(), ds.last_requeued_samples(), ds.last_kernel_ms()
    W, H = 48, 40
    I = PC.frame(W, H, 9, True)
    with ds.glare(W, H) as gl, ds.tone(W, H) as t, ds.psf(W, H, 9) as g:
        glare_before = gl.apply(I)
        t.load(I)
        t.meter()
        codes_before = t.encode()
        gi, ti = bytes(gl.info()), t.info().loads
        g.load(PC.kernel(9, 5))
        for form in FORMS:
            g.apply(I, form=form)
        assert launches() == la and ds.last_requeued_samples() == ra and ds.last_kernel_ms() == ms
        assert gl.info().applies == 1 and t.info().loads == ti and bytes(gl.info())[:32] == gi[:32]
        assert np.array_equal(t.encode(), codes_before)
        assert glare_ref.same_bits(gl.apply(I), glare_before)
    b, sb = ds.render(cam, p)
    assert glare_ref.same_bits(b, a) and launches() == la and sb.clamped_samples == sa.clamped_samples


# ---------------------------------------------------------------- 6. the command-line tool's psf argument
def test_cli_psf_argument(device, host_scenes, tmp_path, emu):
    import subprocess
    import glare_ref
    from test_gpu_aov import _read_pfm
    from test_gpu_tone import read_ppm
    from vecchio_amd import build
    cli = build.build_cli()
    # (aov_spp = 1 writes the float frame, output_0000.pfm; display = 3: ACES; then glare, scale, psf)
    base = ["cornell_box", "64", "16", "20", "1", "1", "1", "1", "0", "0", "0", "3"]
    dirs = {}
    for key, extra in (("absent", []), ("off", ["0", "0", "0"]), ("star", ["0", "0", "6"]), ("both", ["40", "0", "6"])):
        dirs[key] = tmp_path / key
        dirs[key].mkdir()
        subprocess.run([cli] + base + extra, cwd=dirs[key], check=True, timeout=300, capture_output=True)
    names = sorted(f.name for f in dirs["absent"].iterdir())
    assert sorted(f.name for f in dirs["off"].iterdir()) == names
    assert sorted(f.name for f in dirs["star"].iterdir()) == sorted(names + ["output_0000_psf.pfm"])
    assert sorted(f.name for f in dirs["both"].iterdir()) == sorted(names + ["output_0000_glare.pfm", "output_0000_psf.pfm"])
    for n in names:
        assert (dirs["absent"] / n).read_bytes() == (dirs["off"] / n).read_bytes(), n
        if n != "output_0000_display.ppm":
            assert (dirs["absent"] / n).read_bytes() == (dirs["star"] / n).read_bytes(), n
    lib = ffi.load_device_lib()
    star = Psf.star(65, 6, 0.0, 8.0, 0.1, lib=lib)
    frame = _read_pfm(dirs["star"] / "output_0000.pfm")
    want = EMU.apply(frame, star, 0.15, 0.0)
    assert R.same_floats(_read_pfm(dirs["star"] / "output_0000_psf.pfm"), want)
    glared = glare_ref.apply(frame, 6, f32(40) / f32(100), 1.0, 0.0)
    assert glare_ref.same_bits(_read_pfm(dirs["both"] / "output_0000_glare.pfm"), glared)        # the stage sits behind glare
    assert R.same_floats(_read_pfm(dirs["both"] / "output_0000_psf.pfm"), EMU.apply(glared, star, 0.15, 0.0))
    assert subprocess.run([cli] + base + ["0", "0", "65"], cwd=tmp_path, capture_output=True, timeout=60).returncode == 1
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    try:
        with ds.tone(64, 64) as t:
            t.load(want)
            t.meter()
            codes = t.encode()
        assert np.array_equal(read_ppm(dirs["star"] / "output_0000_display.ppm"), codes.astype(np.int64))
        assert not np.array_equal(read_ppm(dirs["absent"] / "output_0000_display.ppm"), codes.astype(np.int64))
    finally:
        ds.close()
