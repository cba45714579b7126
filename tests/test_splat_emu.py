"""Reconstruction filters on the CPU: the kernels' own footprint code (vk_splat.h splat_weights, built with g++ into tests/emu) against
tests/splat_ref.py's numpy restatement of the header's definition — sums, weight sums and the device counters, bit for bit, for every
filter setting on every frame: every pixel pattern with the deposit's special radiances, anchors in the corners and on the edges,
xi = 0 exactly, and caller-supplied positions on pixel boundaries, at -0.0, at `width` exactly and at NaN.  BOX at radius 0.5 against
tests/film_ref.py and tests/exact_sums.py.  A pixel that received negative lobes only."""
import numpy as np
import pytest

import emu_splat_ffi as EMU
import exact_sums as E
import film_ref as F
import splat_ref as R
from vecchio_amd import ffi

f32 = np.float32
N = 257
CASES = [(sp, fr) for sp in R.FILTERS for fr in R.FRAMES]
CASE_IDS = [f"{i}-{w}x{h}" for i in R.FILTER_IDS for w, h in R.FRAMES]


def mixed_status(n):
    """every depositing status, with the others (skipped) at fixed strides"""
    st = np.array([ffi.VK_SHADE_MISS, ffi.VK_SHADE_ENDED, ffi.VK_PATHS_CULLED], np.uint32)[np.arange(n) % 3]
    st[5::31] = ffi.VK_SHADE_SCATTERED
    st[9::43] = ffi.VK_SHADE_BAD_HIT
    return st


def both(states, status, W, H, spp, sp, positions=None, sums=None):
    want, wc = R.deposit(states, status, W, H, spp, sp, positions, sums)
    got, gc = EMU.deposit(states, status, W, H, spp, sp, positions, sums)
    return want, wc, got, gc


def test_the_zero_streams_are_zero(oracle):
    assert oracle.draws(*R.ZERO_X, 0, 2)[0] == 0.0 and oracle.draws(*R.ZERO_Y, 0, 2)[1] == 0.0


@pytest.mark.parametrize("sp,frame", CASES, ids=CASE_IDS)
def test_emulator_equals_the_restatement(sp, frame, oracle):
    W, H = frame
    seen = dict.fromkeys(R.COUNTERS, 0)
    for spp in (3, 40):
        budget = spp * R.side(sp[1]) ** 2                  # the special radiances straddle THIS clamp
        for name, pixel in F.pixel_patterns(N, W * H).items():
            states = R.states_with_samples(pixel, F.radiances(N, budget, seed=len(name)), seed=7)
            want, wc, got, gc = both(states, mixed_status(N), W, H, spp, sp)
            what = f"{sp} {W}x{H} spp {spp} {name}"
            assert np.array_equal(got, want), what
            assert gc == wc, (what, gc, wc)
            for k in seen:
                seen[k] += wc[k]
    assert all(seen.values()), seen
    # anchors in the corners, on the edges and inside, several samples each; and the two streams that start with xi = 0
    pixel = np.repeat(R.anchors(W, H), 8)
    states = R.states_with_samples(pixel, F.radiances(len(pixel), 3, seed=3), seed=11)
    zero = F.states_for(np.zeros(2, np.uint32), np.array([[0.25, 0.5, 1.0], [1.5, 0.125, 2.0]], f32))
    zero["seed"], zero["sample"] = (R.ZERO_X[0], R.ZERO_Y[0]), (R.ZERO_X[2], R.ZERO_Y[2])
    states = np.concatenate([states, zero])
    status = np.full(len(states), ffi.VK_SHADE_MISS, np.uint32)
    want, wc, got, gc = both(states, status, W, H, 3, sp)
    assert np.array_equal(got, want) and gc == wc, (sp, frame, gc, wc)
    full = R.side(sp[1]) ** 2
    assert wc["contributions"] <= wc["deposited"] * full
    if W >= 5 and H >= 5:
        assert wc["contributions"] < wc["deposited"] * full or full == 1      # the corners lose part of their footprint
    # xi = 0 under the half-open box: the sample stays in its own pixel
    if sp[:2] == (R.BOX, 0.5):
        alone, c = R.deposit(zero, status[:2], W, H, 3, sp)
        assert c["contributions"] == 2 and alone[0, 0, 3] == 2 << 26 and alone[..., 3].sum() == 2 << 26


@pytest.mark.parametrize("sp,frame", CASES, ids=CASE_IDS)
def test_positions(sp, frame, oracle):
    W, H = frame
    pos = R.boundary_positions(W, H)
    n = len(pos)
    # state.pixel is not read with positions: every one lies outside the frame here
    states = R.states_with_samples(np.full(n, W * H + 5, np.uint32), F.radiances(n, 3, seed=n), seed=2)
    status = mixed_status(n)
    status[:24] = ffi.VK_PATHS_CULLED
    want, wc, got, gc = both(states, status, W, H, 3, sp, pos)
    assert np.array_equal(got, want) and gc == wc, (sp, frame, gc, wc)
    placed = R.place(states, status, W, H, pos)[0]
    assert list(placed[:9]) == [True, True, True, W > 1 and H > 1, True, True, False, False, False]        # -0.0 is pixel 0; `width` is outside
    assert not placed[9:15].any() and wc["skipped"] >= 9 and wc["deposited"] > 0
    # added to what is there
    again, ac = EMU.deposit(states, status, W, H, 3, sp, pos, sums=got)
    assert np.array_equal(again, 2 * want) and ac == wc


def test_box_half_is_the_film(oracle):
    W, H, spp = 21, 13, 4
    sp = R.FILTERS[0]
    pixel, sample = F.ids_of(W, 0, 0, W, H, 0, spp)
    n = len(pixel)
    acc = F.radiances(n, spp, seed=1)
    status = np.full(n, ffi.VK_SHADE_ENDED, np.uint32)
    states = F.states_for(pixel, acc, seed=9)
    states["sample"] = sample
    film, fc = F.deposit(states, status, W, H, spp)
    sums, c = R.deposit(states, status, W, H, spp, sp)
    assert np.array_equal(sums[..., :3], film)
    assert {k: c[k] for k in fc} == fc and c["contributions"] == c["deposited"] and c["dropped"] > 0 and c["clamped"] > 0
    count = np.zeros(W * H, np.int64)
    np.add.at(count, pixel[np.isfinite(acc).all(axis=1)].astype(np.int64), 1)
    assert np.array_equal(sums[..., 3], count.reshape(H, W) << 26)
    # with every sample finite the weight plane is spp * 2^26 and the resolve is the film's at spp
    acc[~np.isfinite(acc).all(axis=1)] = f32(0.375)
    states["acc"] = acc
    film, _ = F.deposit(states, status, W, H, spp)
    sums, _ = R.deposit(states, status, W, H, spp, sp)
    assert (sums[..., 3] == spp << 26).all() and np.array_equal(sums[..., :3], film)
    assert R.resolve(sums).tobytes() == E.resolve(film, spp).tobytes()
    esums, _ = EMU.deposit(states, status, W, H, spp, sp)
    assert np.array_equal(esums, sums)


def test_negative_lobes_alone_resolve_to_black(oracle):
    W = H = 7
    sp = R.FILTERS[6]                                      # b = 0, c = 0.5: negative between t = 1 and 2
    states = F.states_for(np.zeros(1, np.uint32), np.array([[1.0, 2.0, 0.5]], f32))
    status = np.array([ffi.VK_SHADE_MISS], np.uint32)
    pos = np.array([[2.75, 3.5]], f32)
    sums, c = R.deposit(states, status, W, H, 1, sp, pos)
    esums, ec = EMU.deposit(states, status, W, H, 1, sp, pos)
    assert np.array_equal(esums, sums) and ec == c and c["contributions"] == 16
    assert sums[3, 1, 3] < 0 and sums[3, 4, 3] < 0 and sums[3, 2, 3] > 0 and (sums[3, 1, :3] < 0).all()
    img = R.resolve(sums)
    assert not img[sums[..., 3] <= 0].any() and (img[sums[..., 3] > 0] > 0).all()
    zero_weight = np.array([[[5 << 26, -3 << 26, 1, 0], [5 << 26, 5 << 26, 5 << 26, -1]]], np.int64)
    assert not R.resolve(zero_weight).any()
