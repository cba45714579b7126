"""-m gpu: the laws of guided upsampling through the public calls, in the PLAIN and the TILED form: tests/upsample_laws_ref.py's (a)
constant, (b) linear reproduction, (c) edges with its power control, (d) demodulation and (e) variance with its power control, with the
bounds derived there (32.0001 u, at most 48.1 u, 32.0001 u, 35.0001 u; a chi-square interval at a false-alarm rate of 1e-6)."""
import numpy as np
import pytest

import upsample_laws_ref as L
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMS = {"plain": ffi.VK_UPSAMPLE_FORM_PLAIN, "tiled": ffi.VK_UPSAMPLE_FORM_TILED}


@pytest.fixture(scope="module")
def scene(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    yield ds
    ds.close()


@pytest.fixture(params=sorted(FORMS))
def apply(request, scene):
    """upsample_ref.apply's signature over the device: a handle per pair of sizes, kept until the test ends"""
    handles = {}

    def run(color, W, H, stderr3=None, albedo=None, normal=None, depth=None, albedo_hi=None, normal_hi=None, depth_hi=None,
            want_stderr=True, **params):
        h, w = color.shape[:2]
        if (w, h, W, H) not in handles:
            handles[(w, h, W, H)] = scene.upsample(w, h, W, H)
            handles[(w, h, W, H)].set_form(FORMS[request.param])
        u = handles[(w, h, W, H)]
        u.load(color, stderr3, albedo, normal, depth)
        out, se = u.apply(albedo_hi, normal_hi, depth_hi, want_stderr=want_stderr, **params)
        info = u.info()
        assert info.last_form == FORMS[request.param]
        return out, se, int(info.fallback_pixels), int(info.empty_pixels)

    yield run
    for u in handles.values():
        u.close()


def test_a_constant(apply):
    for shape in L.SHAPES:
        assert L.law_constant(apply, shape) <= 32.001


def test_b_linear_reproduction(apply):
    seen = 0
    for shape in L.SHAPES:
        n, worst, rel = L.law_linear(apply, shape)
        assert worst <= 1.0 and rel <= 48.1
        seen += n
    assert seen > 500


def test_c_edges(apply):
    for shape in ((9, 7, 31, 23), (8, 6, 16, 12), (5, 4, 37, 29), (7, 5, 16, 11), (9, 7, 9, 7)):
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
