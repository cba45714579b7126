"""The f64 laws of the point-spread stage (tests/psf_laws_ref.py) on the CPU: on the numpy restatement and on the host build of
vk_psf.h.  (a) against a direct f64 convolution and numpy.fft in f64; (b) a delta kernel; (c) one interior impulse and the frame's sum;
(d) no wrap-around, and the power of that check against a circular convolution; (e) three channel kernels act independently; (f)
linearity in strength.  u = 2^-24; every bound is derived in psf_laws_ref from the roundings of m_x + m_y stages, the product and the
inverse, and none is tuned to what is measured (DESIGN.md records both)."""
import numpy as np
import pytest

import emu_psf_ffi as EMU
import psf_laws_ref as L
import psf_ref as R


def appliers(emu):
    return {"restatement": R.apply, "host build": EMU.apply}


@pytest.mark.parametrize("which", ["restatement", "host build"])
def test_the_laws(which, emu):
    fig = L.run_all(appliers(emu)[which])
    for key, v in fig.items():
        print("PSF_LAW", which, key, v)
    assert len(fig) == 5 * len(L.LAW_SHAPES) + 2


def test_the_bound_is_what_the_derivation_says():
    """the pieces of the bound: eta = mu + gamma_4 (sqrt 2 + mu), E = m eta / (1 - m eta), and the chain's first-order size"""
    u = L.u
    assert u == 2.0 ** -24
    E = L.transform_error(32, 32)
    eta = u * (1 + 2.0 ** -20) + (4 * u / (1 - 4 * u)) * (2 ** 0.5 + u * (1 + 2.0 ** -20))
    assert E == 10 * eta / (1 - 10 * eta) and 6.6 * u < eta < 6.7 * u
    # a delta frame and a delta kernel: b2 = k2 = S = 1, so dC = E (1 + dG) + dG + p (1 + E)(1 + dG) + E (1 + E)(1 + dG)(1 + p), dG = 32 E
    B = np.zeros((24, 24, 3), np.float32)
    B[3, 4] = 1.0
    k = np.zeros((9, 9, 3), np.float32)
    k[4, 4] = 1.0
    dG, p = 32 * E, 2 ** 0.5 * (2 * u / (1 - 2 * u))
    want = E * (1 + dG) + dG + p * (1 + E) * (1 + dG) + E * (1 + E) * (1 + dG) * (1 + p)
    assert np.allclose(L.conv_bound(24, 24, k, B), want, rtol=1e-12)


def test_the_yardsticks_agree_with_each_other():
    """the direct convolution and numpy.fft, both f64, share no code and agree to f64 rounding"""
    I, k = L.positive_frame(37, 11, 5), R.normalise(L.random_kernel(5, 6))
    a, b = L.conv_direct(I, k), L.conv_numpy_fft(I, k)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    # and the circular convolution differs from the linear one only within K - 1 of the border
    c = L.conv_direct(I, k, period=True)
    assert np.array_equal(c[2:-2, 2:-2], a[2:-2, 2:-2]) and not np.array_equal(c, a)


def test_transform_roundtrip_within_its_bound(emu):
    for Px, Py in ((2, 2), (64, 16), (512, 256), (4096, 4)):
        rng = np.random.default_rng(Px + Py)
        a = rng.normal(0, 1, (Py, Px, 2)).astype(np.float32)
        back = EMU.fft2(EMU.fft2(a), inverse=True)
        assert np.abs(back.astype(np.float64) - a).max() <= L.roundtrip_bound(Px, Py, a)
