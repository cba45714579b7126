"""-m gpu: vk_psf_* beside a caller's non-blocking stream.  No vk_psf function takes a stream: the work is enqueued on the null stream, which a
non-blocking stream does not order against.  The documented duty (vecchio_amd.h "point-spread function", State): the caller synchronises
the stream first, calls, and waits for the null stream afterwards.  Here the frame and the kernel are produced on such a stream behind
other work of that stream, the stream is synchronised, the kernel is loaded and the frame convolved in place, the null stream is waited
for, and the stream carries on with the result: it equals the host build's, in both forms."""
import numpy as np
import pytest

import emu_psf_ffi as EMU
import psf_cases as PC
import psf_ref as R
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu


def test_apply_device_beside_a_non_blocking_stream(device, host_scenes, emu):
    import torch
    hs, cam = host_scenes("cornell_box")
    W, H, K = 61, 7, 5
    I, k = PC.frame(W, H, 31, True), PC.kernel(K, 31)
    want = EMU.apply(I, k, 0.4, 0.5)
    S = torch.cuda.Stream()                                  # non-blocking: unordered against the null stream
    ds = DeviceScene(hs.desc)
    try:
        with ds.psf(W, H, K) as g:
            for form in (ffi.VK_PSF_FORM_PLAIN, ffi.VK_PSF_FORM_LDS):
                host_in, host_k = torch.from_numpy(I).pin_memory(), torch.from_numpy(k).pin_memory()
                with torch.cuda.stream(S):
                    busy = torch.ones(1 << 20, device="cuda")
                    for _ in range(8):
                        busy = busy * 1.0001                 # the stream has work in front of the copies
                    d = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
                    d_k = torch.empty((K, K, 3), dtype=torch.float32, device="cuda")
                    d.copy_(host_in, non_blocking=True)
                    d_k.copy_(host_k, non_blocking=True)
                S.synchronize()                              # the caller's duty: first
                g.load_device(K, d_k)
                g.apply_device(d, strength=0.4, threshold=0.5, form=form)
                torch.cuda.default_stream().synchronize()    # and afterwards: the null stream
                with torch.cuda.stream(S):
                    out = (d * 1.0).cpu()
                S.synchronize()
                assert R.same_floats(out.numpy(), want), form
    finally:
        ds.close()
