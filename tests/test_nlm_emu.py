"""Non-local means on the CPU.  RESTATEMENT: the host build of vk_nlm.h (tests/emu/emu_nlm.cpp) equals tests/nlm_ref.py bit for bit (a
NaN's payload aside), out and stderr3_out, on 1x1, 1x7, 7x1, 5x5 (smaller than a patch and a window), 33x9 and 65x17, R in {1, 3, 10} x F
in {0, 1, 3}, with and without albedo, stderr3_out wanted or not, and on the special inputs of nlm_ref.special_cases.  PROPERTIES of the
host build with bounds that follow from the definition.  QUALITY: on a Cornell box the oracle rendered, the restatement's output at the
shipped defaults is closer to a 8192-spp reference than the noisy frame is."""
import numpy as np
import pytest

import emu_nlm_ffi as EMU
import nlm_ref as R

f32 = np.float32
SIZES = [(1, 1), (1, 7), (7, 1), (5, 5), (33, 9), (65, 17)]
RADII = [(r, f) for r in (1, 3, 10) for f in (0, 1, 3)]
EPS = 2.0 ** -24


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_host_build_equals_the_restatement(size, emu):
    W, H = size
    color, se, albedo = R.synthetic(W, H, seed=100 * W + H)
    for r, f in RADII:
        for alb in (albedo, None):
            want, want_se = R.filter(color, se, alb, r, f, 0.45, 1.0, 1e-3)
            got, got_se = EMU.filter(color, se, alb, r, f, 0.45, 1.0, 1e-3)
            assert R.same_bits(got, want) and R.same_bits(got_se, want_se), (size, r, f, alb is None)
            only, none = EMU.filter(color, se, alb, r, f, 0.45, 1.0, 1e-3, want_stderr=False)
            assert none is None and R.same_bits(only, want)
    # other parameters: k, alpha, the floor
    want, want_se = R.filter(color, se, albedo, 3, 1, 0.9, 0.25, 0.5)
    got, got_se = EMU.filter(color, se, albedo, 3, 1, 0.9, 0.25, 0.5)
    assert R.same_bits(got, want) and R.same_bits(got_se, want_se)


@pytest.mark.parametrize("size", [(5, 5), (33, 9), (65, 17)], ids=["5x5", "33x9", "65x17"])
def test_special_inputs(size, emu):
    W, H = size
    cases = R.special_cases(W, H, seed=3)
    assert sorted(cases) == ["albedo_zero", "nonfinite_block", "nonfinite_single", "overflow", "plain", "zero_stderr"]
    for name, (color, se, albedo) in cases.items():
        for r, f in ((3, 1), (10, 3)):
            want, want_se = R.filter(color, se, albedo, r, f)
            got, got_se = EMU.filter(color, se, albedo, r, f)
            assert R.same_bits(got, want) and R.same_bits(got_se, want_se), (size, name, r, f)
            bad = ~(np.isfinite(color).all(axis=2) & np.isfinite(se).all(axis=2))
            assert R.same_bits(got[bad], color[bad]) and R.same_bits(got_se[bad], se[bad]), (size, name)
            if name in ("plain", "albedo_zero"):
                assert np.isfinite(got).all() and np.isfinite(got_se).all()
    if size == (65, 17):
        # the special paths are walked: the floor, a patch distance of +inf and one that is no number
        color, se, albedo = cases["albedo_zero"]
        assert (albedo < 1e-3).any()
        with np.errstate(all="ignore"):
            I, V, Vf, a, valid = R.prepare(*cases["zero_stderr"], 1e-3)
            assert (Vf[:, :20] == 0).all() and np.isinf((I[1, 0] - I[0, 0]) ** 2 / f32(1e-10)).all()
            I, V, Vf, a, valid = R.prepare(*cases["overflow"], 1e-3)
            assert np.isinf(Vf[0, 0]).all() and np.isnan((I[0, 0] - I[0, 1]) ** 2 - Vf[0, 0]).all()


def test_constant_image_stays_constant(emu):
    """every tap carries the same I, so J / W is a weighted mean of one value: each of the T = (2R + 1)^2 products w * c and each of the T
    additions into J round once, W likewise, and the division once — |out - c| <= (T + 2) 2^-24 |c| covers the relative error of a sum
    of T positive terms (at most (T - 1) 2^-24 to first order) plus the product's and the quotient's"""
    rng = np.random.default_rng(5)
    W, H = 23, 11
    c = np.broadcast_to(np.array([0.7, 1.3, 2.9], f32), (H, W, 3)).copy()
    se = (rng.random((H, W, 3)) * 0.5).astype(f32)
    se[3:6, 4:9] = 0.0
    for r, f in ((1, 0), (3, 1), (7, 3), (10, 3)):
        out, _ = EMU.filter(c, se, None, r, f)
        T = (2 * r + 1) ** 2
        assert (np.abs(out.astype(np.float64) - c) <= (T + 2) * EPS * np.abs(c)).all(), (r, f)


def test_nothing_crosses_a_noiseless_step_edge(emu):
    """two levels, stderr 1e-6 * level: a pair across the edge has d * d = 4 over a denominator of about 1e-10, so its offset's weight is
    E(something enormous) = 0; every tap with weight carries the pixel's own level and the bound of the constant image holds"""
    W, H = 24, 12
    c = np.empty((H, W, 3), f32)
    c[:, : W // 2] = 1.0
    c[:, W // 2:] = 3.0
    se = (c * f32(1e-6)).astype(f32)
    for r, f in ((3, 1), (7, 3), (10, 3)):
        out, _ = EMU.filter(c, se, None, r, f)
        T = (2 * r + 1) ** 2
        assert (np.abs(out.astype(np.float64) - c) <= (T + 2) * EPS * np.abs(c)).all(), (r, f)


def test_invalid_pixels_pass_and_their_values_touch_nothing_else(emu):
    W, H = 33, 9
    color, se, albedo = R.synthetic(W, H, seed=8)
    a, b = color.copy(), color.copy()
    sa, sb = se.copy(), se.copy()
    a[4, 16] = (np.nan, 1.0, 2.0)
    b[4, 16] = (5.0, np.inf, -7.0)
    sa[2, 3, 0] = np.inf
    sb[2, 3] = (np.nan, 123.0, -np.inf)
    for r, f in ((3, 1), (10, 3)):
        oa, ea = EMU.filter(a, sa, albedo, r, f)
        ob, eb = EMU.filter(b, sb, albedo, r, f)
        bad = np.zeros((H, W), bool)
        bad[4, 16] = bad[2, 3] = True
        assert R.same_bits(oa[bad], a[bad]) and R.same_bits(ea[bad], sa[bad]) and R.same_bits(ob[bad], b[bad]) and R.same_bits(eb[bad], sb[bad])
        assert np.array_equal(oa[~bad].view(np.uint32), ob[~bad].view(np.uint32))
        assert np.array_equal(ea[~bad].view(np.uint32), eb[~bad].view(np.uint32))


def test_rotation_where_the_order_allows_it(emu):
    """a 2 x 1 frame and its rotation, 1 x 2: every sum of the definition has at most two terms (the centre and the one neighbour), and a
    sum of two terms does not depend on their order.  Nothing of the kind holds for a larger frame: the offset order is not symmetric."""
    color = np.array([[[0.5, 1.0, 2.0], [0.6, 0.9, 2.2]]], f32)
    se = np.array([[[0.1, 0.2, 0.3], [0.2, 0.1, 0.4]]], f32)
    for r, f in ((1, 0), (3, 1), (10, 3)):
        o1, e1 = EMU.filter(color, se, None, r, f)
        o2, e2 = EMU.filter(color.transpose(1, 0, 2), se.transpose(1, 0, 2), None, r, f)
        assert R.same_bits(e1.transpose(1, 0, 2), e2) and R.same_bits(o1.transpose(1, 0, 2), o2)


def test_stderr_out_is_bounded_by_the_window_maximum(emu):
    """U / W^2 <= max V over the taps (a convex combination of V with weights w^2 / W^2 that add up to at most 1); in f32 the T products
    and T additions of U, the square root, W's additions and the division each round once: a factor 1 + (2T + 4) 2^-24 covers them"""
    W, H = 33, 17
    color, se, _ = R.synthetic(W, H, seed=12)
    for r, f in ((1, 0), (3, 1), (10, 3)):
        _, out = EMU.filter(color, se, None, r, f)
        T = (2 * r + 1) ** 2
        window = np.zeros_like(se)
        for oy in range(-r, r + 1):
            for ox in range(-r, r + 1):
                window = np.maximum(window, R.shift(se, ox, oy, f32(0)))
        assert (out.astype(np.float64) <= window.astype(np.float64) * (1 + (2 * T + 4) * EPS)).all(), (r, f)


# ---------------------------------------------------------------- quality, with the oracle
QUALITY_SIZE = 32              # (64 x 64 halved: the 8192-spp reference of 64 x 64 takes the oracle eight seconds)
QUALITY_R = 0.388              # the restatement's ratio at the shipped defaults, measured once (DESIGN.md "Non-local means")


def oracle_frame(oracle, host_scenes, size=QUALITY_SIZE, spp=16, windows=4):
    """Cornell at 16 spp in 4 windows: the mean, the batch-means standard error (vk_progress_stderr's formula, in f64) and a reference at
    8192 spp of another seed"""
    hs, cam = host_scenes("cornell_box")
    img, ps = oracle.render_samples(hs.desc, cam, hs.params(size, spp, 50, seed=5, height=size))
    ps = ps[:, :3].reshape(size, size, windows, spp // windows, 3).astype(np.float64)
    m = ps.mean(axis=3)
    mean = ps.mean(axis=(2, 3))
    n = spp // windows
    var = ((n * m * m).sum(axis=2) - spp * mean * mean) / ((windows - 1) * spp)
    ref, _ = oracle.render(hs.desc, cam, hs.params(size, 8192, 50, seed=99, height=size))
    return img, np.sqrt(np.maximum(var, 0.0)).astype(f32), ref


def test_quality_on_the_oracles_cornell_box(oracle, host_scenes):
    img, se, ref = oracle_frame(oracle, host_scenes)
    out, _ = R.filter(img, se)                      # the shipped defaults: R 7, F 3, k 0.45, alpha 1
    ratio = R.rel_mse(out, ref) / R.rel_mse(img, ref)
    print(f"relMSE noisy {R.rel_mse(img, ref):.5f} nlm {R.rel_mse(out, ref):.5f} ratio {ratio:.4f}")
    assert ratio < 1
    assert ratio <= 1 - (1 - QUALITY_R) / 2, ratio
