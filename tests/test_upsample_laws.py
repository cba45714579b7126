"""The laws of guided upsampling on the CPU: tests/upsample_laws_ref.py's (a) constant, (b) linear reproduction, (c) edges with its power
control, (d) demodulation and (e) variance with its power control, on the numpy restatement and on the host build of vk_upsample.h.

The derived bounds (upsample_laws_ref.py's docstring): (a) and (c) 32.0001 u, (d) 35.0001 u relative, u = 2^-24; (b) an absolute
tolerance per pixel that is at most 48.1 u of the value on these shapes; all below 64 u.  (e): 800 draws, 27 pixel-components, a false-alarm
rate of 1e-6 for the whole law: s^2 / r^2 within [0.7015, 1.3430]; a stderr3_out too large by 1.5 lies 11 sigma outside."""
import numpy as np
import pytest

import emu_upsample_ffi as EMU
import upsample_laws_ref as L
import upsample_ref as R

f32 = np.float32
APPLY = {"restatement": R.apply, "host-build": EMU.apply}


@pytest.fixture(params=sorted(APPLY))
def apply(request, emu):
    return APPLY[request.param]


def test_the_bounds_are_the_derived_ones():
    assert L.BOUND_CONSTANT == L.g(32) and L.BOUND_DEMODULATION == L.g(35)
    assert 32 * L.U < L.BOUND_CONSTANT < 32.001 * L.U and L.BOUND_DEMODULATION < 35.001 * L.U < 64 * L.U
    for shape in L.SHAPES:
        tol, v = L.linear_bound(shape)
        m = L.interior(*shape)
        if m.any():
            assert (tol[m] / np.abs(v[m])).max() <= L.LINEAR_WORST < 64 * L.U, (shape, (tol[m] / np.abs(v[m])).max() / L.U)
    k = L.VAR_DRAWS - 1
    lo, hi = L.chi2_interval(k)
    assert abs(lo / k - 0.7015) < 1e-3 and abs(hi / k - 1.3430) < 1e-3
    assert (lo - k / 2.25) / (np.sqrt(2 * k) / 2.25) > 11


@pytest.mark.parametrize("shape", L.SHAPES, ids=["%dx%d-%dx%d" % s for s in L.SHAPES])
def test_a_constant(apply, shape):
    assert L.law_constant(apply, shape) <= 32.001


def test_b_linear_reproduction(apply):
    seen = 0
    for shape in L.SHAPES:
        n, worst, rel = L.law_linear(apply, shape)
        assert worst <= 1.0 and rel <= 48.1
        seen += n
    # (2x2 -> 5x5 has no interior pixel; the others have)
    assert seen > 500 and L.law_linear(apply, (2, 2, 5, 5))[0] == 0


@pytest.mark.parametrize("shape", [(9, 7, 31, 23), (8, 6, 16, 12), (5, 4, 37, 29), (7, 5, 16, 11), (9, 7, 9, 7)],
                         ids=lambda s: "%dx%d-%dx%d" % s)
def test_c_edges(apply, shape):
    err, off = L.law_edges(apply, shape)
    assert err <= 32.001 and off > 1.0


def test_d_demodulation(apply):
    for shape in ((8, 6, 16, 12), (9, 7, 31, 23), (9, 7, 9, 7)):
        assert L.law_demodulation(apply, shape) <= 35.001


def test_e_variance(apply):
    _, _, W, H = L.VAR_SHAPE
    draws, se = L.variance_draws()
    outs = np.empty((L.VAR_DRAWS, H, W, 3), f32)
    rep = None
    for i, c in enumerate(draws):
        outs[i], r, fb, _ = apply(c, W, H, stderr3=se)
        assert fb == 0 and (rep is None or np.array_equal(r, rep))
        rep = r
    stats = L.law_variance(outs, rep)
    assert 0.7 < min(stats) and max(stats) < 1.35
