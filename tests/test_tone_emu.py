"""The display transform on the CPU.  vk_tone_solve (host code of the library, no device) against tests/tone_ref.py's restatement in
Python floats, bit for bit: empty, single-bin, two-bin and random histograms, fractions that cut inside a bin, blend chains of three
frames, clamping; the 0.21-octave bound of the metered exposure against the true trimmed geometric mean of log-normal images.  The
kernels' own per-pixel code (vk_tone.h through g++, tests/emu) against the numpy restatement, bit for bit: the histogram, and every curve
x transfer x dither on the special values and on noise.  Contract 6: the codes against the f64 closed form on 2 * 10^6 inputs."""
import ctypes as C
import math

import numpy as np
import pytest

import emu_tone_ffi as EMU
import tone_ref as T
from vecchio_amd import ffi

f32 = np.float32
COMBOS = [(c, t, d) for c in T.CURVES for t in T.TRANSFERS for d in (False, True) if not (d and t == T.REFERENCE)]
WHITE = {T.CLAMP: 11.2, T.REINHARD: 4.0, T.HABLE: 11.2, T.ACES: 11.2}


def meter_params(**kw):
    mp = ffi.ToneMeterParams(0.18, 0.10, 0.02, 1.0, -16.0, 16.0, (0, 0))
    for k, v in kw.items():
        setattr(mp, k, v)
    return mp


def lib_solve(bins, mp, prev=None):
    lib = ffi.load_device_lib()
    bins = np.ascontiguousarray(bins, np.uint32)
    info = ffi.ToneMeterInfo(9.0, 9.0, 9, 9, 9, 9, 9.0, 9)
    p = None if prev is None else C.byref(C.c_double(prev))
    assert lib.vk_tone_solve(bins.ctypes.data, C.byref(mp), p, C.byref(info)) == ffi.VK_OK, lib.vk_last_error()
    assert (info.below, info.above, info.nonfinite) == (0, 0, 0)
    return T.info_dict(info)


def library_table(transfer):
    tab = np.zeros(510, f32)
    assert ffi.load_device_lib().vk_debug_tone_table(transfer, tab.ctypes.data) == ffi.VK_OK
    return tab


def histograms():
    rng = np.random.default_rng(11)
    out = {"empty": np.zeros(640, np.uint32)}
    for b in (0, 1, 319, 320, 639):
        h = np.zeros(640, np.uint32)
        h[b] = 1 + b
        out[f"single_{b}"] = h
    h = np.zeros(640, np.uint32)
    h[100], h[500] = 900, 100
    out["two"] = h
    h = np.zeros(640, np.uint32)
    h[7], h[8] = 3, 5                                            # 8 pixels: every default fraction cuts inside a bin
    out["two_adjacent"] = h
    out["one_pixel"] = np.eye(1, 640, 333, dtype=np.uint32)[0]
    out["full"] = np.full(640, 0xFFFFFFFF, np.uint32)            # N = 640 * (2^32 - 1): beyond any frame, exact in f64 all the same
    for k in range(12):
        h = np.zeros(640, np.uint32)
        n = int(rng.integers(1, 640))
        h[rng.choice(640, n, replace=False)] = rng.integers(1, 1 << int(rng.integers(1, 28)), n)
        out[f"random_{k}"] = h
    centre = rng.normal(320, 40, 20000).astype(int).clip(0, 639)
    out["bell"] = np.bincount(centre, minlength=640).astype(np.uint32)
    return out


FRACTIONS = [(0.10, 0.02), (0.0, 0.0), (0.5, 0.49), (0.10, 0.15), (1.0 / 3.0, 1.0 / 3.0), (0.0, 0.99), (0.99, 0.0), (1e-9, 1e-9)]


def test_solve_equals_the_restatement(built):
    seen_cut = 0
    for name, h in histograms().items():
        for low, high in FRACTIONS:
            for prev in (None, -3.25, 17.0):
                for blend in (1.0, 0.25, 0.0):
                    mp = meter_params(low_fraction=low, high_fraction=high, blend=blend)
                    got, want = lib_solve(h, mp, prev), T.solve(h, mp, prev)
                    assert T.same_info(got, want), (name, low, high, prev, blend, got, want)
        N = int(h.astype(np.uint64).sum())
        seen_cut += N > 0 and (0.10 * N) % 1 != 0
    assert seen_cut > 5
    # what the cases must show: empty keeps 1.0f (or the previous exposure); a single bin's target is its centre whatever the fractions
    e = lib_solve(np.zeros(640, np.uint32), meter_params())
    assert e["flags"] == ffi.VK_TONE_METER_EMPTY and e["exposure"] == 1.0 and e["log2_used"] == 0.0 and e["binned"] == 0
    e = lib_solve(np.zeros(640, np.uint32), meter_params(), prev=2.0)
    assert e["flags"] == ffi.VK_TONE_METER_EMPTY and e["log2_used"] == 2.0 and e["exposure"] == f32(0.18) / f32(4.0)
    one = np.zeros(640, np.uint32)
    one[320] = 1000                                               # [1, 2^(1/16)): centre 1/32 octave
    s = lib_solve(one, meter_params(low_fraction=0.3, high_fraction=0.3))
    assert s["flags"] == 0 and s["log2_target"] == s["log2_used"] == 1.0 / 32.0 and s["binned"] == 1000
    assert s["exposure"] == f32(float(f32(0.18)) * math.ldexp(1.0 + (1.0 - 1.0 / 32.0), -1))
    # two bins, 90 % dark and 10 % bright: the trim drops the bright ones
    two = np.zeros(640, np.uint32)
    two[304], two[516] = 900, 100                                 # 0.5 and ~5000
    trimmed = lib_solve(two, meter_params(low_fraction=0.10, high_fraction=0.15))
    untrimmed = lib_solve(two, meter_params(low_fraction=0.0, high_fraction=0.0))
    assert trimmed["log2_target"] == -20 + 304.5 / 16 and untrimmed["log2_target"] > trimmed["log2_target"] + 1.0
    assert abs(0.5 * float(trimmed["exposure"]) - 0.177) < 0.004 and abs(0.5 * float(untrimmed["exposure"]) - 0.074) < 0.004


def test_blend_chains_and_clamping(built):
    hs = histograms()
    chain = [hs["bell"], hs["two"], hs["random_3"], hs["empty"], hs["single_639"]]
    for blend in (0.25, 0.5, 1.0, 0.0):
        mp = meter_params(blend=blend)
        prev_lib = prev_ref = None
        for k, h in enumerate(chain):
            got, want = lib_solve(h, mp, prev_lib), T.solve(h, mp, prev_ref)
            assert T.same_info(got, want), (blend, k)
            if not got["flags"]:
                prev_lib, prev_ref = got["log2_used"], want["log2_used"]
            if k == 1 and blend == 0.25:
                first = T.solve(chain[0], mp)["log2_used"]
                assert got["log2_used"] == first + float(f32(0.25)) * (got["log2_target"] - first)
            if k >= 1 and blend == 0.0:
                assert got["log2_used"] == T.solve(chain[0], mp)["log2_used"]
    # clamping: at both ends, with and without a previous exposure; the exposure is the clamped one's
    for h, lo, hi in ((hs["single_0"], -3.0, 5.0), (hs["single_639"], -3.0, 5.0), (hs["bell"], 0.0, 0.0), (hs["bell"], -1.0, -0.5)):
        for prev in (None, 4.0, -40.0):
            mp = meter_params(min_log2=lo, max_log2=hi, blend=0.5)
            got, want = lib_solve(h, mp, prev), T.solve(h, mp, prev)
            assert T.same_info(got, want) and lo <= got["log2_used"] <= hi
            assert got["exposure"] == f32(float(f32(0.18)) * T.pexp2(-got["log2_used"]))
    assert lib_solve(hs["single_0"], meter_params(min_log2=-3.0, max_log2=5.0))["log2_used"] == -3.0
    assert lib_solve(hs["single_639"], meter_params(min_log2=-3.0, max_log2=5.0))["log2_used"] == 5.0


def test_the_metered_exposure_is_within_0_21_octave_of_the_key(built):
    """200 log-normal images (mean -10 .. 8 octaves, sd 0 .. 3): exposure * (the trimmed geometric mean of the luminance, the trim cut
    between the sorted pixels with fractional weights) lies within 0.21 octave of key — 0.0861 for the piecewise-linear log, 0.0861 for
    the piecewise-linear exp, 1/32 for a bin's centre"""
    rng = np.random.default_rng(5)
    worst = 0.0
    for k in range(200):
        mean, sd = rng.uniform(-10, 8), rng.uniform(0, 3)
        low, high = ((0.10, 0.02), (0.0, 0.0), (0.25, 0.25), (0.10, 0.15))[k % 4]
        grey = np.exp2(rng.normal(mean, sd, 4096)).astype(f32)
        rgb = np.repeat(grey[:, None], 3, axis=1)
        bins, counters = T.histogram(rgb)
        assert counters[0] == 4096
        mp = meter_params(low_fraction=low, high_fraction=high, key=0.18)
        s = lib_solve(bins, mp)
        Y = np.sort(np.log2(T.luminance(rgb[:, 0], rgb[:, 1], rgb[:, 2]).astype(np.float64)))
        i = np.arange(4096, dtype=np.float64)
        lo, hi = float(f32(low)) * 4096, (1.0 - float(f32(high))) * 4096
        w = np.maximum(0.0, np.minimum(i + 1, hi) - np.maximum(i, lo))
        true = float((w * Y).sum() / w.sum())
        err = abs(math.log2(float(s["exposure"])) + true - math.log2(float(f32(0.18))))
        worst = max(worst, err)
        assert err <= 0.21, (k, mean, sd, low, high, err)
    print(f"worst error {worst:.4f} octave")


def test_the_emulated_histogram_equals_the_restatement(emu):
    frames = [T.specials(library_table(T.SRGB)), T.noise(37, 23, 1).reshape(-1, 3), T.noise(64, 64, 2, -25, 25).reshape(-1, 3),
              np.full((1000, 3), 0.18, f32)]
    for rgb in frames:
        bins, counters = EMU.histogram(rgb)
        want_bins, want_counters = T.histogram(rgb)
        assert np.array_equal(bins, want_bins) and np.array_equal(counters, want_counters)
        assert int(counters.sum()) == len(rgb) and int(bins.sum()) == int(counters[0])
    bins, counters = T.histogram(frames[0])
    assert counters.all() and bins[0] > 0 and bins[639] > 0           # every counter and both end bins are met by the specials
    # the edges: 2^-20 is bin 0, its lower neighbour below; 2^20 is above, its lower neighbour bin 639 (as pure green of that luminance
    # the value is not exact: grey with weights that sum to 1 in f32 up to rounding is what the specials hold, so probe Y directly)
    for y, where in ((2.0 ** -20, 0), (2.0 ** -19, 16), (1.0, 320), (np.nextafter(f32(2.0 ** 20), f32(0)), 639)):
        assert (int(np.array(f32(y)).view(np.uint32)) >> 19) - T.BIN_BASE == where


@pytest.mark.parametrize("curve,transfer,dither", COMBOS, ids=[f"c{c}_t{t}_d{int(d)}" for c, t, d in COMBOS])
def test_the_emulated_encode_equals_the_restatement(curve, transfer, dither, emu, built):
    table = None if transfer == T.REFERENCE else library_table(transfer)
    p = T.curve_param(curve, WHITE[curve])
    if curve == T.HABLE:
        assert EMU.hable(WHITE[curve]).tobytes() == f32(p).tobytes()
    sp = T.specials(table)
    frames = [(T.frame_of(sp, 61, -(-len(sp) // 61)), 1.0), (T.frame_of(sp, 5, 3), 0.37), (T.noise(37, 23, 3), 1.0), (T.noise(1, 1, 4), 2.5),
              (T.noise(64, 16, 5, -12, 6), 0.18)]
    for rgb, E in frames:
        for seed in ((0, 0xDEADBEEFCAFE) if dither else (0,)):
            got = EMU.encode(rgb, curve, table, dither, E, p, seed)
            want = T.encode(rgb, curve, table, dither, E, p, seed)
            assert got.shape == want.shape == rgb.shape and np.array_equal(got, want), (rgb.shape, E, seed, np.argwhere(got != want)[:4])
    if curve == T.REINHARD:                                           # white = +inf: the plain x / (1 + Y)
        rgb = T.noise(16, 16, 6, -12, 6)
        pinf = T.curve_param(curve, np.inf)
        assert np.isinf(pinf) and np.array_equal(EMU.encode(rgb, curve, table, dither, 1.0, pinf, 3), T.encode(rgb, curve, table, dither, 1.0, pinf, 3))


def test_dither_draws_are_the_stream_generator_s(emu):
    """the restatement of rng_for_stream / gen_f32 against the host library's generator through the emulated encode: on a frame set
    exactly between two codes, a pixel's code is base + (u < fr) for the restated u"""
    table = library_table(T.SRGB)
    base = 100
    lo, hi = table[2 * base - 1], table[2 * base + 1]
    y = f32(lo + (hi - lo) * f32(0.5))
    rgb = np.full((32, 32, 3), y, f32)
    got = EMU.encode(rgb, T.CLAMP, table, True, 1.0, 0.0, seed=77)
    u = T.dither_draws(77, np.arange(1024)).reshape(32, 32, 3)[::-1]
    fr = f32(f32(y - lo) / f32(hi - lo))
    assert np.array_equal(got, (base + (u < fr)).astype(np.uint8)) and 0.4 < (got == base + 1).mean() < 0.6
    assert not np.array_equal(got, EMU.encode(rgb, T.CLAMP, table, True, 1.0, 0.0, seed=78))


def test_identity_is_to_color(emu):
    """CLAMP + REFERENCE + E = 1: Vec3::to_color's bytes on the values it is known by (vec3.rs:44-61: sqrt, clamp at 0.999, * 256)"""
    vals = np.array([0.0, -0.0, 1.0, 0.25, 0.998001, 4.0, -1.0, np.nan, np.inf, -np.inf, 1e-40, 0.5], f32)
    rgb = np.repeat(vals[:, None], 3, axis=1).reshape(1, -1, 3)
    want = [0, 0, 255, 128, 255, 255, 0, 0, 255, 0, 0, 181]
    for enc in (EMU.encode, T.encode):
        assert enc(rgb, T.CLAMP, None, False, 1.0, 0.0)[0, :, 0].tolist() == want


@pytest.mark.parametrize("curve", T.CURVES)
def test_codes_against_the_closed_form(curve, emu, built):
    """contract 6 on 2 * 10^6 log-uniform inputs over -12 .. 6 octaves: against round(255 * OETF(curve(E * x))) in f64 no component is
    off by more than one code and at most 1e-4 of them by one (the restatement measured 3.5e-6 for ACES, 8e-6 for Hable, 1e-6 for
    Reinhard, 0 without a curve when the definition was written: the cap is ten times the worst)"""
    n = 2_000_000 // 3 + 1
    rgb = T.noise(n, 1, 9 + curve, -12.0, 6.0)
    p = T.curve_param(curve, WHITE[curve])
    for transfer in (T.SRGB, T.GAMMA22):
        table = library_table(transfer)
        for E in (1.0, 0.18):
            got = EMU.encode(rgb, curve, table, False, E, p)
            if E == 1.0:
                assert np.array_equal(got, T.encode(rgb, curve, table, False, E, p))
            want = T.closed_form(rgb.reshape(-1, 3), curve, transfer, E, WHITE[curve])
            diff = np.abs(got.reshape(-1, 3).astype(np.int64) - want)
            share = float((diff == 1).mean())
            print(f"curve {curve} transfer {transfer} E {E}: off by one {share:.2e} of {diff.size}")
            assert diff.max() <= 1 and share <= 1e-4, (curve, transfer, E, int(diff.max()), share)
            assert len(np.unique(got)) > 200                          # (the inputs reach the whole range of codes)
