"""Glare on the CPU.  RESTATEMENT: the host build of vk_glare.h (tests/emu/emu_glare.cpp) equals tests/glare_ref.py bit for bit (a NaN's
payload aside) on 1x1, 2x3, 5x1, 37x53, 64x32 and 130x70, L in {1, 2, 3, 6, 8}, falloff 0.5, 1 and 2, threshold 0 and 1, on random HDR
frames sown with NaN, +-inf, -0, negatives and values above 2^20; the weights and the launch plan.  PROPERTIES of the restatement with
bounds that follow from the definition or from the f64 operator: bit equality carries them to the host build and to the device."""
import numpy as np
import pytest

import emu_glare_ffi as EMU
import glare_ref as R

f32, f64 = np.float32, np.float64
SIZES = [(1, 1), (2, 3), (5, 1), (37, 53), (64, 32), (130, 70)]
LEVELS = (1, 2, 3, 6, 8)
FALLOFFS = (0.5, 1.0, 2.0)
THRESHOLDS = (0.0, 1.0)


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_host_build_equals_the_restatement(size, emu):
    W, H = size
    I = R.hdr_frame(W, H, seed=100 * W + H)
    assert not np.isfinite(I).all() or W * H < 11
    for L in LEVELS:
        for fo in FALLOFFS:
            for th in THRESHOLDS:
                want = R.apply(I, L, 0.3, fo, th)
                got = EMU.apply(I, L, 0.3, fo, th)
                assert R.same_bits(got, want), (size, L, fo, th, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4].tolist())
                # a component that is not finite stays what it was
                bad = ~np.isfinite(I)
                assert R.same_bits(got[bad], I[bad])
    for st in (0.0, 0.15, 1.0):
        assert R.same_bits(EMU.apply(I, 6, st, 1.0, 0.25), R.apply(I, 6, st, 1.0, 0.25))


def test_weights_and_launch_plan(emu):
    for L in range(1, 9):
        for fo in (0.5, 1.0, 2.0, 0.3, 7.5):
            c = EMU.weights(L, fo)
            assert np.array_equal(c, np.array(R.weights(L, fo), f32)), (L, fo)
            assert abs(float(c.astype(f64).sum()) - 1.0) <= L * 2.0 ** -24
    assert np.array_equal(EMU.weights(4, 1.0), np.full(4, 0.25, f32))
    # PLAIN launches max(1, 2L - 2) kernels; FUSED strictly fewer from L = 3 on, at every size (the form codes: 1 PLAIN, 2 FUSED)
    for W, H in SIZES + [(256, 144), (317, 301), (321, 311), (800, 800), (900, 900), (1920, 1080), (4096, 1), (65535, 3)]:
        for L in range(1, 9):
            plain, fused = EMU.launch_count(W, H, L, 1), EMU.launch_count(W, H, L, 2)
            assert plain == max(1, 2 * L - 2)
            assert fused < plain if L >= 3 else fused == plain, (W, H, L, plain, fused)
    # the tail takes over from the first level >= 1 whose upper planes fit its LDS: 8192, 6144 and 1792 floats per component
    assert [EMU.tail_level(*s) for s in ((130, 70), (256, 144), (317, 301), (321, 311), (900, 900), (1920, 1080))] == [1, 1, 1, 2, 3, 4]
    assert EMU.launch_count(1920, 1080, 6, 2) == 8 and EMU.launch_count(317, 301, 8, 2) == 3 and EMU.launch_count(321, 311, 8, 2) == 4


# ---------------------------------------------------------------- the closed-form properties, on the restatement
def test_identity():
    for W, H in SIZES:
        I = R.hdr_frame(W, H, seed=7 * W + H)
        fin = np.isfinite(I)
        for out in (R.apply(I, 1, 0.8, 1.0, 0.0), R.apply(I, 1, 1.0, 2.0, 1.0), R.apply(I, 6, 0.0, 1.0, 0.0), R.apply(I, 8, 0.0, 0.5, 1.0)):
            assert np.array_equal(out[fin], I[fin]) and R.same_bits(out[~fin], I[~fin])          # as floats: a -0 is +0
    assert R.apply(np.full((1, 1, 3), -0.0, f32), 1, 1.0)[0, 0].view(np.uint32).tolist() == [0, 0, 0]


def test_constant_frame():
    """A constant frame stays constant: every filter's taps sum to 8/8 or 4/4 and the weights to 1.  Measured on the f32 restatement
    against the constant, over the sizes above, L in {1, 2, 3, 5, 6, 8}, the values below and strength 0.15 and 1: 1 ulp of the constant
    at the most (the f64 operator: 0.5 ulp, from the weights' rounding); the bound is four times that."""
    worst = 0.0
    for W, H in SIZES + [(19, 23)]:
        for L in (1, 2, 3, 5, 6, 8):
            for v in (0.7, 1.0, 3.3, 1e-3, 150.0):
                for st in (0.15, 1.0):
                    out = R.apply(np.full((H, W, 3), v, f32), L, st, 1.0, 0.0)
                    worst = max(worst, float(np.abs(out.astype(f64) - f64(f32(v))).max() / np.spacing(f32(v))))
    print(f"constant frame: worst deviation {worst} ulp")
    assert worst <= 4.0


ENERGY_CASES = [(37, 53, 3), (144, 256, 5), (130, 70, 4)]
ENERGY_F32 = 5.1e-8          # the worst relative difference of sum(A_0) and sum(I) the f32 restatement shows on these cases (falloff 0.5, 1, 2)


def test_energy_and_linearity():
    worst = 0.0
    for W, H, L in ENERGY_CASES:
        I = R.lamp_frame(W, H, 1, L)
        total = float(I.astype(f64).sum())
        for fo in FALLOFFS:
            A64, B64 = R.spread(I.astype(f64), L, fo, 0.0, f64)
            assert abs(float(A64.sum()) - total) <= 1e-12 * total and float(B64.sum()) == total, (W, H, L, fo)
            A32, _ = R.spread(I, L, fo, 0.0)
            worst = max(worst, abs(float(A32.astype(f64).sum()) - total) / total)
            # what the output as a whole gains or loses is the same share, times strength
            out = R.apply(I, L, 0.15, fo, 0.0)
            assert abs(float(out.astype(f64).sum()) - total) / total <= 4 * ENERGY_F32
        # linearity: scaling by 2 is exact in f32 (no overflow past 2^20, no subnormals)
        for st in (0.15, 1.0):
            assert R.same_bits(R.apply(I * f32(2), L, st, 1.0, 0.0), R.apply(I, L, st, 1.0, 0.0) * f32(2)), (W, H, L, st)
    print(f"energy: worst relative difference of the f32 sums {worst:.3e}")
    assert worst <= 4 * ENERGY_F32


def test_mirror():
    """64 x 32, L = 5: every level's size is even until it is 4 x 2, so the taps of a flipped frame are the flipped taps and the outer
    additions of down4 commute; the up filter's pairs are mirror images of each other"""
    for special, th in ((False, 0.0), (True, 1.0)):
        I = R.hdr_frame(64, 32, 5, special=special)
        out = R.apply(I, 5, 0.4, 1.0, th)
        assert R.same_bits(R.apply(I[:, ::-1], 5, 0.4, 1.0, th), out[:, ::-1])
        assert R.same_bits(R.apply(I[::-1], 5, 0.4, 1.0, th), out[::-1])
        assert R.same_bits(R.apply(I[::-1, ::-1], 5, 0.4, 1.0, th), out[::-1, ::-1])


# the RMS radius of an impulse's A_0 in f64 (falloff 1): the restatement's own figures, pinned
RMS_RADIUS = {2: 1.224744871391589, 4: 4.5, 6: 15.049916943292411}


def test_impulse():
    I = np.zeros((257, 257, 3), f64)
    I[128, 128] = 1.0
    y, x = np.mgrid[0:257, 0:257]
    r2 = (x - 128.0) ** 2 + (y - 128.0) ** 2
    last = 0.0
    for L in (1, 2, 3, 4, 5, 6):
        A, B = R.spread(I, L, 1.0, 0.0, f64)
        a = A[..., 0]
        assert a.min() >= 0.0 and abs(float(a.sum()) - 1.0) <= 1e-12 and np.array_equal(A[..., 1], a)
        radius = float(np.sqrt((a * r2).sum() / a.sum()))
        assert radius > last or L == 1
        last = radius
        if L in RMS_RADIUS:
            assert abs(radius - RMS_RADIUS[L]) <= 1e-6 * RMS_RADIUS[L], (L, radius)
        # strength 1: the output is A_0 itself, but for the rounding of I + (A_0 - B) at the impulse
        assert np.abs(R.apply(I, L, 1.0, 1.0, 0.0, f64) - A).max() <= 2.0 ** -52


F32_AGAINST_F64 = 3.19e-6    # max |out32 - out64| / max(out64) over the frames below: strength 1, where I - B cancels (DESIGN.md "Glare")


def test_f32_against_the_f64_operator():
    worst = 0.0
    for W, H in SIZES:
        I = R.hdr_frame(W, H, seed=100 * W + H, special=False)
        for L in LEVELS:
            for fo in FALLOFFS:
                for th in THRESHOLDS:
                    for st in (0.15, 1.0):
                        a = R.apply(I, L, st, fo, th).astype(f64)
                        b = R.apply(I.astype(f64), L, st, fo, th, f64)
                        worst = max(worst, float(np.abs(a - b).max() / b.max()))
    print(f"f32 against f64: worst {worst:.3e} of the frame's maximum")
    assert worst <= 4 * F32_AGAINST_F64
