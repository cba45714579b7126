"""-m gpu: the f64 laws of the point-spread stage (tests/psf_laws_ref.py: (a) against a direct f64 convolution and numpy.fft, (b) a delta
kernel, (c) an impulse, (d) no wrap-around, with its power control, (e) independent channels, (f) linearity in strength) through the public
calls on the MI355X, in the PLAIN and the LDS form.  The bounds are psf_laws_ref's, derived there from the arithmetic."""
import numpy as np
import pytest

import psf_laws_ref as L
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    yield ds
    ds.close()


@pytest.mark.parametrize("form", [ffi.VK_PSF_FORM_PLAIN, ffi.VK_PSF_FORM_LDS], ids=["plain", "lds"])
def test_the_laws_through_the_public_calls(form, scene):
    handles = {}

    def apply(I, kernel, strength, threshold):
        H, W = I.shape[:2]
        key = (W, H, kernel.shape[0])
        if key not in handles:
            handles[key] = scene.psf(*key)
        g = handles[key]
        g.load(kernel)
        return g.apply(I, strength=strength, threshold=threshold, form=form)

    try:
        fig = L.run_all(apply)
    finally:
        for g in handles.values():
            g.close()
    for key, v in fig.items():
        print("PSF_LAW", form, key, v)
    assert len(fig) == 5 * len(L.LAW_SHAPES) + 2
