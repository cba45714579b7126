"""The display transform on the device.  HISTOGRAM: bins and counters equal tests/tone_ref.py's restatement in both kernel forms on 1x1,
4x1, 5x3, 37x23 (width not a multiple of 4, rows straddled) and 257x129 (more than one workgroup, a tail) frames of special values, of
log-uniform noise over 30 octaves and of one flat colour (every lane on one bin).  METER: vk_tone_meter's info is vk_tone_solve's and
the restatement's, over three frames with blend 0.25 and a reset.  IDENTITY: CLAMP + REFERENCE + 1.0f is vk_to_color_device's bytes and
vk_render's VK_OUTPUT_RGB8 frame.  ENCODE: every curve x transfer x dither equals the restatement and the host build bit for bit;
contract 6 on the 257x129 noise frame; the dither's properties; device pointers; refusals; the CLI's trailing argument."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_tone_ffi as EMU
import tone_ref as T
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (4, 1), (5, 3), (37, 23), (257, 129)]
SHAPE_IDS = [f"{w}x{h}" for w, h in SHAPES]
COMBOS = [(c, t, d) for c in T.CURVES for t in T.TRANSFERS for d in (False, True) if not (d and t == T.REFERENCE)]
WHITE = {T.CLAMP: 11.2, T.REINHARD: 4.0, T.HABLE: 11.2, T.ACES: 11.2}
FORMS = (ffi.VK_TONE_FORM_LDS, ffi.VK_TONE_FORM_PLAIN)


@pytest.fixture(scope="module")
def scene(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    yield ds
    ds.close()


@pytest.fixture(scope="module")
def tables(built):
    out = {T.REFERENCE: None}
    for transfer in (T.SRGB, T.GAMMA22):
        tab = np.zeros(510, f32)
        assert ffi.load_device_lib().vk_debug_tone_table(transfer, tab.ctypes.data) == ffi.VK_OK
        out[transfer] = tab
    return out


def contents(W, H, tables):
    """the frames of one shape: the special values (rotated so that a small frame holds the non-finite ones), noise over 30 octaves, flat"""
    sp = T.specials(tables[T.SRGB])
    return {"specials": T.frame_of(sp, W, H), "specials_tail": T.frame_of(sp[::-1], W, H), "noise": T.noise(W, H, W * 1000 + H),
            "flat": np.full((H, W, 3), 0.18, f32)}


def encode_params(curve, transfer, dither=False, metered=False, exposure=1.0, seed=0):
    flags = (ffi.VK_TONE_DITHER if dither else 0) | (ffi.VK_TONE_USE_METERED if metered else 0)
    return ffi.ToneParams(curve, transfer, flags, 0, exposure, WHITE[curve], seed)


def meter_params(**kw):
    mp = ffi.ToneMeterParams(0.18, 0.10, 0.02, 1.0, -16.0, 16.0, (0, 0))
    for k, v in kw.items():
        setattr(mp, k, v)
    return mp


def lib_solve(lib, bins, mp, prev):
    info = ffi.ToneMeterInfo()
    p = None if prev is None else C.byref(C.c_double(prev))
    assert lib.vk_tone_solve(np.ascontiguousarray(bins, np.uint32).ctypes.data, C.byref(mp), p, C.byref(info)) == ffi.VK_OK
    return T.info_dict(info)


# ---------------------------------------------------------------- 1. histogram
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_histogram_and_counters_are_exact_in_both_forms(shape, scene, tables, emu):
    W, H = shape
    with scene.tone(W, H) as t:
        for name, rgb in contents(W, H, tables).items():
            want_bins, want_counters = T.histogram(rgb)
            emu_bins, emu_counters = EMU.histogram(rgb)
            assert np.array_equal(emu_bins, want_bins) and np.array_equal(emu_counters, want_counters)
            t.load(rgb)
            for form in FORMS:
                t.set_form(form)
                info = t.meter()
                bins, counters = t.histogram()
                assert np.array_equal(bins, want_bins), (name, form, np.argwhere(bins != want_bins)[:4])
                assert np.array_equal(counters, want_counters), (name, form, counters, want_counters)
                assert (info.binned, info.below, info.above, info.nonfinite) == tuple(int(c) for c in want_counters), (name, form)
                assert int(counters.sum()) == W * H
            if name == "flat":
                assert int(want_bins.max()) == W * H                # the contention case: every pixel in one bin
        assert t.last_ms()[0] > 0


# ---------------------------------------------------------------- 2. meter
def test_meter_is_solve_of_the_histogram_over_three_frames_and_a_reset(scene, tables):
    lib = scene._lib
    W, H = 37, 23
    frames = [T.noise(W, H, 1, -6, 2), T.noise(W, H, 2, 0, 9), T.noise(W, H, 3, -12, -4), np.zeros((H, W, 3), f32)]
    mp = meter_params(blend=0.25, low_fraction=0.1, high_fraction=0.15)
    with scene.tone(W, H) as t:
        for round_ in range(2):
            prev = None
            for k, rgb in enumerate(frames):
                t.load(rgb)
                info = t.meter(mp)
                bins, counters = t.histogram()
                got = T.info_dict(info)
                assert T.same_info(got, lib_solve(lib, bins, mp, prev)) and T.same_info(got, T.solve(bins, mp, prev)), (round_, k)
                if k == 3:                                        # a black frame: EMPTY, the exposure stays, and is no previous meter
                    assert got["flags"] == ffi.VK_TONE_METER_EMPTY and got["log2_used"] == prev and info.below == W * H
                else:
                    assert got["flags"] == 0
                    if k:
                        assert got["log2_used"] == prev + float(f32(0.25)) * (got["log2_target"] - prev)
                    else:
                        assert got["log2_used"] == got["log2_target"]                  # a first meter (after create, after reset)
                    prev = got["log2_used"]
                ti = t.info()
                assert ti.exposure == info.exposure and ti.metered == 1 and ti.log2_used == prev
                assert (ti.width, ti.height, ti.loads, ti.meters) == (W, H, round_ * 4 + k + 1, round_ * 4 + k + 1)
            t.reset()
            ti = t.info()
            assert (ti.metered, ti.exposure, ti.log2_used) == (0, 1.0, 0.0)
        # a first meter of a black frame: exposure 1.0f, EMPTY, and USE_METERED is admitted with it
        t.load(frames[3])
        info = t.meter(mp)
        assert info.flags == ffi.VK_TONE_METER_EMPTY and info.exposure == 1.0 and t.info().metered == 1
        assert not t.encode(encode_params(T.ACES, T.SRGB, metered=True)).any()


# ---------------------------------------------------------------- 3. identity
def test_identity_is_to_color_device_and_the_rgb8_render(scene, tables, host_scenes):
    import torch
    identity = encode_params(T.CLAMP, T.REFERENCE)
    for W, H in ((37, 23), (5, 3), (64, 9)):
        for name, rgb in contents(W, H, tables).items():
            d_rgb = torch.from_numpy(rgb).cuda()
            d_out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            scene.to_color_device(d_rgb.data_ptr(), W, H, d_out.data_ptr())
            torch.cuda.synchronize()
            with scene.tone(W, H) as t:
                t.load(rgb)
                got = t.encode(identity)
            assert np.array_equal(got, d_out.cpu().numpy()), (W, H, name)
            assert np.array_equal(got, T.encode(rgb, T.CLAMP, None, False, 1.0, 0.0))
    hs, cam = host_scenes("cornell_box")
    img, _ = scene.render(cam, hs.params(32, 16, 12, seed=4))
    img8, _ = scene.render(cam, hs.params(32, 16, 12, seed=4, output_format=ffi.VK_OUTPUT_RGB8))
    with scene.tone(32, 32) as t:
        t.load(img)
        assert np.array_equal(t.encode(identity), img8)
        # the Cornell frame's histogram in both forms, and the frame through the whole transform: metered, ACES, sRGB
        want_bins, want_counters = T.histogram(img)
        for form in FORMS:
            t.set_form(form)
            info = t.meter()
            bins, counters = t.histogram()
            assert np.array_equal(bins, want_bins) and np.array_equal(counters, want_counters), form
        assert T.same_info(T.info_dict(info), T.solve(bins, meter_params()))
        want = T.encode(img, T.ACES, tables[T.SRGB], False, info.exposure, 0.0)
        assert np.array_equal(t.encode(encode_params(T.ACES, T.SRGB, metered=True)), want)
        assert info.exposure > 1.0 and want.mean() > img8.mean()    # a dark room under one small lamp: the meter opens up


# ---------------------------------------------------------------- 4. every combination
@pytest.mark.parametrize("curve,transfer,dither", COMBOS, ids=[f"c{c}_t{t}_d{int(d)}" for c, t, d in COMBOS])
def test_every_combination_equals_the_restatement_and_the_host_build(curve, transfer, dither, scene, tables, emu):
    table = tables[transfer]
    p = T.curve_param(curve, WHITE[curve])
    for W, H in SHAPES:
        with scene.tone(W, H) as t:
            for name, rgb in contents(W, H, tables).items():
                if name == "flat":
                    continue
                t.load(rgb)
                for exposure, seed in ((1.0, 0), (0.37, 0x1234567890ABCDEF)):
                    got = t.encode(encode_params(curve, transfer, dither, exposure=exposure, seed=seed))
                    want = T.encode(rgb, curve, table, dither, exposure, p, seed)
                    assert np.array_equal(got, want), (W, H, name, exposure, np.argwhere(got != want)[:4])
                    assert np.array_equal(got, EMU.encode(rgb, curve, table, dither, exposure, p, seed)), (W, H, name, exposure)
            # metered: E = params.exposure * the metered exposure, in f32
            rgb = T.noise(W, H, 7, -9, 3)
            t.load(rgb)
            info = t.meter()
            E = f32(f32(0.5) * f32(info.exposure))
            got = t.encode(encode_params(curve, transfer, dither, metered=True, exposure=0.5, seed=5))
            assert np.array_equal(got, T.encode(rgb, curve, table, dither, E, p, 5)), (W, H)
            assert t.last_ms()[1] > 0


def test_reinhard_with_an_infinite_white(scene, tables):
    rgb = T.noise(37, 23, 8, -12, 6)
    tp = ffi.ToneParams(T.REINHARD, T.SRGB, 0, 0, 1.0, float("inf"), 0)
    with scene.tone(37, 23) as t:
        t.load(rgb)
        assert np.array_equal(t.encode(tp), T.encode(rgb, T.REINHARD, tables[T.SRGB], False, 1.0, f32(np.inf)))


# ---------------------------------------------------------------- 5. contract 6
@pytest.mark.parametrize("curve", T.CURVES)
def test_codes_against_the_closed_form(curve, scene, tables):
    """the 257 x 129 noise frame, -12 .. 6 octaves: 99 459 components, none off by more than one code, at most 1e-4 of them (nine) by one"""
    W, H = 257, 129
    rgb = T.noise(W, H, 40 + curve, -12.0, 6.0)
    with scene.tone(W, H) as t:
        t.load(rgb)
        for transfer in (T.SRGB, T.GAMMA22):
            got = t.encode(encode_params(curve, transfer))
            want = T.closed_form(rgb.reshape(-1, 3), curve, transfer, 1.0, WHITE[curve]).reshape(H, W, 3)[::-1]
            diff = np.abs(got.astype(np.int64) - want)
            print(f"curve {curve} transfer {transfer}: {int((diff == 1).sum())} of {diff.size} off by one")
            assert diff.size == 99459 and diff.max() <= 1 and (diff == 1).mean() <= 1e-4, (curve, transfer, int(diff.max()), int((diff == 1).sum()))


# ---------------------------------------------------------------- 6. dither
def test_dither(scene, tables):
    W, H = 257, 129
    table = tables[T.SRGB]
    base = 120
    lo, hi = table[2 * base - 1], table[2 * base + 1]
    y = f32(lo + f32(hi - lo) * f32(0.3))
    fr = float(f32(f32(y - lo) / f32(hi - lo)))
    flat = np.full((H, W, 3), y, f32)
    noise = T.noise(W, H, 9, -8, 2)
    with scene.tone(W, H) as t:
        t.load(noise)
        a = t.encode(encode_params(T.ACES, T.SRGB, True, seed=11))
        assert np.array_equal(a, t.encode(encode_params(T.ACES, T.SRGB, True, seed=11)))          # the same seed, a second encode
        other = t.encode(encode_params(T.ACES, T.SRGB, True, seed=12))
        assert not np.array_equal(a, other) and np.abs(a.astype(int) - other.astype(int)).max() <= 1
        plain = t.encode(encode_params(T.ACES, T.SRGB, False))
        assert np.abs(a.astype(int) - plain.astype(int)).max() <= 1
        for form in FORMS:                                            # the meter's form has no say
            t.set_form(form)
            t.meter()
            assert np.array_equal(a, t.encode(encode_params(T.ACES, T.SRGB, True, seed=11)))
        t.load(flat)
        codes = t.encode(encode_params(T.CLAMP, T.SRGB, True, seed=3)).astype(np.float64)
        assert set(np.unique(codes)) == {base, base + 1}
        n = codes.size
        sd = np.sqrt(fr * (1 - fr) / n)
        assert abs(codes.mean() - (base + fr)) <= 4 * sd, (codes.mean(), base + fr, sd)


# ---------------------------------------------------------------- 7. device pointers
def test_load_device_and_encode_device(scene, tables):
    import torch
    for W, H in ((37, 23), (257, 129)):
        rgb = T.noise(W, H, 21, -8, 4)
        tp = encode_params(T.HABLE, T.GAMMA22, True, seed=9)
        with scene.tone(W, H) as a, scene.tone(W, H) as b:
            a.load(rgb)
            want = a.encode(tp)
            d_rgb = torch.from_numpy(rgb).cuda()                      # (a blocking copy on the null stream: ordered before the load)
            b.load_device(d_rgb)
            assert np.array_equal(b.encode(tp), want)
            ia, ib = a.meter(), b.meter()
            assert bytes(ia) == bytes(ib)
            d_out = torch.full((H, W, 3), 0x77, dtype=torch.uint8, device="cuda")
            b.encode_device(d_out, tp)
            assert b.last_ms()[1] > 0                                 # (waits for the event behind the encode)
            torch.cuda.synchronize()
            assert np.array_equal(d_out.cpu().numpy(), want)
            b.load_device(d_rgb.data_ptr())                          # a bare pointer
            assert np.array_equal(b.encode(tp), want) and b.info().loads == 2 and b.info().encodes == 3
            # an unaligned output pointer is refused and nothing is written
            d_big = torch.full((W * H * 3 + 8,), 0x55, dtype=torch.uint8, device="cuda")
            assert scene._lib.vk_tone_encode_device(b._h, C.byref(tp), C.c_void_p(d_big.data_ptr() + 1)) == ffi.VK_ERR_BAD_ARG
            assert b"4-byte aligned" in scene._lib.vk_last_error()
            torch.cuda.synchronize()
            assert bool((d_big == 0x55).all())


# ---------------------------------------------------------------- 8. refusals that need a handle, and what a handle owns
def test_refusals_with_a_handle_and_live_objects(device, host_scenes, tables):
    dbg = ffi.load_debug_lib()
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc, lib=dbg)

    def live():
        out = (C.c_uint64 * 4)()
        assert dbg.vk_debug_live_objects(C.byref(out)) == ffi.VK_OK
        return tuple(out)

    try:
        before = live()
        W, H = 5, 3
        t = ds.tone(W, H)
        assert live()[0] == before[0] + 3 and live()[2] == before[2] + 4
        codes = np.full((H, W, 3), 7, np.uint8)
        info = ffi.ToneMeterInfo(9.0, 9.0, 9, 9, 9, 9, 9.0, 9)
        canary = bytes(info)
        ok, mp = encode_params(T.ACES, T.SRGB), meter_params()

        def refused_encode(tp, word):
            assert dbg.vk_tone_encode(t._h, C.byref(tp), codes.ctypes.data) == ffi.VK_ERR_BAD_ARG and word in dbg.vk_last_error(), word
            assert (codes == 7).all()

        refused_encode(ok, b"vk_tone_encode before vk_tone_load")
        assert dbg.vk_tone_meter(t._h, C.byref(mp), C.byref(info)) == ffi.VK_ERR_BAD_ARG and b"vk_tone_meter before vk_tone_load" in dbg.vk_last_error()
        assert bytes(info) == canary
        bins, counters = t.histogram()
        assert not bins.any() and not counters.any()
        t.load(T.noise(W, H, 1))
        refused_encode(encode_params(T.ACES, T.SRGB, metered=True), b"VK_TONE_USE_METERED before vk_tone_meter")
        refused_encode(encode_params(T.ACES, T.REFERENCE, dither=True), b"dither needs a table transfer")
        refused_encode(ffi.ToneParams(9, 1, 0, 0, 1.0, 11.2, 0), b"unknown curve")
        assert dbg.vk_tone_meter(t._h, C.byref(meter_params(blend=2.0)), C.byref(info)) == ffi.VK_ERR_BAD_ARG and bytes(info) == canary
        assert t.info().encodes == 0 and t.info().meters == 0 and t.info().loads == 1
        t.meter()
        assert t.encode(encode_params(T.ACES, T.SRGB, metered=True)).shape == (H, W, 3)
        assert live()[0] == before[0] + 4                            # the codes' buffer, on the first host encode
        t.reset()
        refused_encode(ok, b"vk_tone_encode before vk_tone_load")   # reset forgets the frame
        assert dbg.vk_debug_tone_set_form(t._h, 2) == ffi.VK_ERR_BAD_ARG and b"unknown meter form" in dbg.vk_last_error()
        t.close()
        assert live() == before
        dbg.vk_tone_destroy(None)
    finally:
        ds.close()


# ---------------------------------------------------------------- 9. the CLI
def read_ppm(path):
    toks = path.read_text().split()
    assert toks[0] == "P3" and toks[3] == "255"
    w, h = int(toks[1]), int(toks[2])
    return np.array(toks[4:], np.int64).reshape(h, w, 3)


def test_cli_display_argument(device, host_scenes, tables, tmp_path):
    from test_gpu_aov import _read_pfm
    from vecchio_amd import build
    cli = build.build_cli()
    # (denoise = 1 needs steps >= 2: two windows of the 16 samples, first-hit buffers of 16)
    base = ["cornell_box", "64", "16", "20", "1", "1", "2", "16", "1", "0", "0"]
    dirs = {}
    for key, extra in (("absent", []), ("zero", ["0"]), ("hable", ["2"])):
        dirs[key] = tmp_path / key
        dirs[key].mkdir()
        subprocess.run([cli] + base + extra, cwd=dirs[key], check=True, timeout=300, capture_output=True)
    names = sorted(f.name for f in dirs["absent"].iterdir())
    assert sorted(f.name for f in dirs["zero"].iterdir()) == names
    assert sorted(f.name for f in dirs["hable"].iterdir()) == sorted(names + ["output_0000_display.ppm"])
    for n in names:
        assert (dirs["absent"] / n).read_bytes() == (dirs["zero"] / n).read_bytes() == (dirs["hable"] / n).read_bytes(), n
    clean = _read_pfm(dirs["hable"] / "output_0000_denoised.pfm")
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    try:
        with ds.tone(64, 64) as t:
            t.load(clean)
            info = t.meter()
            want = t.encode(curve=T.HABLE)
        assert np.array_equal(read_ppm(dirs["hable"] / "output_0000_display.ppm"), want.astype(np.int64))
        assert np.array_equal(want, T.encode(clean, T.HABLE, tables[T.SRGB], False, info.exposure, T.curve_param(T.HABLE, 11.2)))
    finally:
        ds.close()
