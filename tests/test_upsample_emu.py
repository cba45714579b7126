"""Guided upsampling on the CPU.  RESTATEMENT: the host build of vk_upsample.h (tests/emu/emu_upsample.cpp) equals tests/upsample_ref.py
bit for bit (a NaN's payload aside) — the frame, stderr3 and the two counts — on the sizes of upsample_cases.CPU_SIZES over
upsample_cases.cases(): every subset of guides, stderr3 on and off, sigma_z 0.5 / 1 / 4, squarings 0 / 3 / 7, low frames with NaN and inf
pixels, misses (depth inf, normal 0), and a block of invalid low pixels that makes both counts non-zero."""
import numpy as np
import pytest

import emu_upsample_ffi as EMU
import upsample_cases as K
import upsample_ref as R

f32 = np.float32


@pytest.mark.parametrize("size", K.CPU_SIZES, ids=["%dx%d-%dx%d" % s for s in K.CPU_SIZES])
def test_host_build_equals_the_restatement(size, emu):
    w, h, W, H = size
    seen_fb = seen_empty = 0
    for name, fkw, g, se, pkw in K.cases():
        fr = K.frame(w, h, W, H, **fkw)
        kw = dict(K.arguments(fr, g, se), **pkw)
        want = R.apply(fr["color"], W, H, **kw)
        got = EMU.apply(fr["color"], W, H, **kw)
        assert K.same(got[0], want[0]), (size, name, np.argwhere(got[0].view(np.uint32) != want[0].view(np.uint32))[:4].tolist())
        assert K.same(got[1], want[1]), (size, name)
        assert got[2:] == want[2:], (size, name, got[2:], want[2:])
        assert want[3] <= want[2] <= W * H
        if name == "block":
            # every high pixel whose 16 taps lie in the block is empty (a frame too small for the block is invalid as a whole)
            assert want[3] > 0 and (want[3] < W * H if w >= 8 and h >= 7 else want[3] == W * H), (size, want[2:])
            assert (want[0].reshape(-1, 3)[(want[1] == 0).all(-1).ravel()] == 0).all()
        seen_fb += want[2]
        seen_empty += want[3]
    # (pixels that fall back and are not empty: a miss among hits, a hit among misses)
    assert seen_empty > 0 and (seen_fb > seen_empty or w < 5)


def test_the_cases_hold_what_they_promise():
    fr = K.frame(13, 11, 40, 33, seed=1, bad=True)
    assert not np.isfinite(fr["color"]).all() and not np.isfinite(fr["stderr3"]).all()
    assert np.isinf(fr["depth"]).any() and (fr["normal"] == 0).all(-1).any() and np.isinf(fr["depth_hi"]).any()
    names = [c[0] for c in K.cases()]
    assert len(set(names)) == len(names) and len({c[2] for c in K.cases()}) == 8
    assert {c[4].get("sigma_z") for c in K.cases()} >= {0.5, 1.0, 4.0} and {c[4].get("normal_squarings") for c in K.cases()} >= {0, 3, 7}


def test_ratios_and_auto(emu):
    for lo, hi in ((2, 2), (2, 5), (7, 16), (9, 9), (960, 1920), (225, 900), (321, 641), (2, 65535)):
        assert EMU.ratios(lo, hi) == R.ratios(lo, hi)
    # the mapping puts the first and last high centres inside the low frame's span, and is monotone
    for lo, hi in ((2, 5), (7, 16), (321, 641), (100, 317)):
        px = R.centres(hi, R.ratios(lo, hi)[0])
        assert (np.diff(px) >= 0).all() and px[0] >= -0.5 and px[-1] <= lo - 1
        assert np.floor(px[31::32] if hi > 32 else px[-1:]).max() - np.floor(px[0]) <= hi
    # AUTO is a function of the sizes alone: the tiled form (2), which was measured faster wherever it was measured (DESIGN.md "Guided
    # upsampling")
    for s in K.CPU_SIZES + [(960, 540, 1920, 1080), (225, 225, 900, 900), (200, 200, 800, 800)]:
        assert EMU.auto_form(*s) == 2


def test_one_side_only_switches_a_term_off(emu):
    """a normal or a depth given at one size only is no error and equals not giving it at all"""
    w, h, W, H = 9, 7, 31, 23
    fr = K.frame(w, h, W, H, seed=5)
    base = R.apply(fr["color"], W, H, stderr3=fr["stderr3"])
    for kw in (dict(normal=fr["normal"]), dict(normal_hi=fr["normal_hi"]), dict(depth=fr["depth"]), dict(depth_hi=fr["depth_hi"])):
        for A in (R, EMU):
            got = A.apply(fr["color"], W, H, stderr3=fr["stderr3"], **kw)
            assert K.same(got[0], base[0]) and K.same(got[1], base[1]) and got[2:] == base[2:], list(kw)
