"""The sample law behind tests/estimator_laws_ref.py, on the oracle and the emulator, and that module's expectations against itself.

1. The law: per-sample renders of the integrating sphere's 16 x 16 frame (test_radiometry.py's routes) at max_depth 3 and 50 — every
   sample is 0 or one Le a^j, the counts per j fit f (1 - f)^(j - 1), the j of neighbouring pixels and of successive samples are
   uncorrelated.  Rules A to E of the reference module stand on this.
2. Every expectation of the reference module on draw() alone — numpy's own generator, no renderer: the f64 side meets its own caps and
   every power control is rejected.  tests/test_gpu_estimator_laws.py holds the public calls to the same functions.
The one statistic a host build exposes (emu_robust_ffi: vk_robust_resolve's per-pixel arithmetic through g++) goes through rule A too."""
import math

import numpy as np
import pytest

import estimator_laws_ref as E
import radiometry_ref as R

f64 = np.float64


# ---------------------------------------------------------------- the closed forms of the law
@pytest.mark.parametrize("D", (2,) + E.DEPTHS)
def test_moments_are_the_geometric_sums(D):
    lw = E.law(D)
    mu, m2 = lw.closed_forms()
    np.testing.assert_allclose(lw.mu, mu, rtol=1e-13)
    np.testing.assert_allclose(lw.m2, m2, rtol=1e-13)
    np.testing.assert_allclose(lw.mu, R.sphere_frame(D).want[0, 0], rtol=1e-13)            # sphere_frame's `want`
    assert abs(lw.probs.sum() + lw.p_zero - 1.0) < 1e-15 and (lw.var > 0).all()


@pytest.mark.parametrize("D", E.DEPTHS)
def test_draw_follows_the_law(D):
    lw = E.law(D)
    x = lw.draw(E.rng_for(0, D), (1 << 20,))
    mean, se = E.ratio(x / lw.mu)
    second, sse = E.ratio(x * x / lw.m2)
    print(f"\n   D{D} draw(): mean / mu {mean} se {se}; second moment ratio {second} se {sse}")
    assert (np.abs(mean - 1) <= E.Z_MAX * se).all() and (np.abs(second - 1) <= E.Z_MAX * sse).all()


# ---------------------------------------------------------------- 1. the law on the oracle and the emulator
def classify(samples, lw):
    """j per sample (0: the zero sample) from (n, >= 3) samples: every one must be 0 or one Le a^j, the same j in all three channels,
    within R.ROUND (relative) — or, past j = 7, within the f32 rounding of the product itself: a sample is Le times j factors a, every
    factor rounded once to f32 and every product rounded once, (2 j + 1) 2^-24 at the most.  (Measured on both routes at max_depth 50:
    within 1e-6 up to j = 36; 1.00e-6 to 1.16e-6 for the six samples of 262 144 with j = 37 .. 42, whose bound is 4.5e-6 to 5.1e-6.)"""
    x = np.asarray(samples, f64)[:, :3]
    assert np.isfinite(x).all()
    tol = np.maximum(R.ROUND, (2.0 * lw.j + 1.0) * 2.0 ** -24)
    near = (np.abs(x[:, None, :] / lw.values[None, :, :] - 1.0) <= tol[None, :, None]).all(2)
    zero = ~x.any(1)
    assert (near.sum(1) + zero == 1).all(), f"{int(((near.sum(1) + zero) != 1).sum())} samples are neither 0 nor one Le a^j"
    return np.where(zero, 0, near.argmax(1) + 1)


def chi_square(j, lw):
    """(chi^2, degrees of freedom, (chi^2 - dof) / sqrt(2 dof)) of the counts per j against f (1 - f)^(j - 1); the zero sample is a
    class of its own, and the tail whose classes expect fewer than 8 is pooled into one"""
    n = len(j)
    expect = np.concatenate([[lw.p_zero], lw.probs]) * n
    count = np.bincount(j, minlength=len(expect)).astype(f64)
    big = expect >= 8.0
    e = np.concatenate([expect[big], [expect[~big].sum()]])
    c = np.concatenate([count[big], [count[~big].sum()]])
    if e[-1] < 8.0:
        e, c = np.concatenate([e[:-2], [e[-2] + e[-1]]]), np.concatenate([c[:-2], [c[-2] + c[-1]]])
    chi2, dof = float(((c - e) ** 2 / e).sum()), len(e) - 1
    return chi2, dof, (chi2 - dof) / math.sqrt(2.0 * dof)


def correlation_z(a, b):
    """r sqrt(n) of two equally long series: N(0, 1) when they are uncorrelated"""
    a, b = np.asarray(a, f64).ravel(), np.asarray(b, f64).ravel()
    return float(np.corrcoef(a, b)[0, 1] * math.sqrt(len(a)))


def check_law(samples, D, what):
    lw = E.law(D)
    case = R.sphere_frame(D)
    w, h = case.size
    j = classify(samples, lw)
    chi2, dof, z = chi_square(j, lw)
    # the path length as the series' value: a zero sample never met the lamp within D - 1 segments
    length = np.where(j == 0, D, j).reshape(h, w, case.spp)
    zx, zy, zs = correlation_z(length[:, :-1], length[:, 1:]), correlation_z(length[:-1], length[1:]), correlation_z(length[..., :-1], length[..., 1:])
    print(f"\n   {what} D{D}: {len(j)} samples, chi^2 {chi2:.1f} on {dof} ({z:+.2f} sigma); correlation z: pixel x+1 {zx:+.2f}, y+1 {zy:+.2f}, "
          f"sample s+1 {zs:+.2f}")
    assert z <= 5.0, f"{what}: the counts per j do not fit f (1 - f)^(j - 1): chi^2 {chi2} on {dof}"
    assert max(abs(zx), abs(zy), abs(zs)) <= E.Z_MAX
    # a frame that follows the law meets rule A: the batch-means variance of its pixels, windows of 256 of its 1024 samples
    x = np.asarray(samples, f64)[:, :3].reshape(h * w, 4, case.spp // 4, 3).sum(2)
    windows = (case.spp // 4,) * 4
    mean, v = E.batch_means(x, windows)
    r = E.rule_a(np.sqrt(np.maximum(v, 0)), lw.var / case.spp, 0.06, f"{what} D{D}")         # (256 pixels: too few to ask a control of)
    print(f"   rule A on its 256 pixels: R {np.round(r[0], 3)} se {np.round(r[1], 3)} z {np.round(r[2], 2)}", end="")


@pytest.mark.parametrize("D", E.DEPTHS)
def test_emulator_samples_follow_the_law(D, emu):
    case = R.sphere_frame(D)
    owner, desc = case.scene()
    check_law(emu.render_samples(desc, case.cam, case.render_params())[1], D, "emulator")


@pytest.mark.parametrize("D", E.DEPTHS)
def test_oracle_samples_follow_the_law(D, oracle):
    case = R.sphere_frame(D)
    owner, desc = case.scene()
    check_law(oracle.render_samples(desc, case.cam, case.render_params())[1], D, "oracle")


# ---------------------------------------------------------------- 2. the reference module's expectations on draw()
def controls_a(windows):
    return [E.control_divisor_k(windows)] + ([E.control_equal_weights(windows)] if len(set(windows)) > 1 else [])


@pytest.mark.parametrize("D", E.DEPTHS)
@pytest.mark.parametrize("plan", list(E.PLANS))
def test_rules_a_and_b_on_draw(plan, D):
    """a frame of the plan's size drawn from numpy: rule A with its controls, rule B against the 2^18-pixel simulation"""
    w, h, windows, cap = E.PLANS[plan]
    lw = E.law(D)
    mean, v = E.batch_means(E.window_sums(lw, E.rng_for(1, D, len(windows), w), w * h, windows), windows)
    se = np.sqrt(np.maximum(v, 0.0))
    r, rse, z, zc = E.rule_a(se, lw.var / sum(windows), cap, f"draw() {plan} D{D}", controls_a(windows))
    got, want, zb, ctrl, zbc, asked = E.rule_b(mean, se, D, plan, f"draw() {plan} D{D}")
    print(f"\n   {plan} D{D}: A R {np.round(r, 4)} se {np.round(rse, 4)} z {np.round(z, 2)} controls {[np.round(c, 1) for c in zc]}; "
          f"B covered {np.round(got, 4)} expected {np.round(want, 4)} z {np.round(zb, 2)} control {np.round(ctrl, 4)} z {np.round(zbc, 2)} "
          f"asked {asked} power {np.round(E.control_power_b(D, plan, w * h), 1)}")
    if plan in ("k2", "equal64", "k8_128"):
        assert asked.any()


def test_equal_weights_control_is_what_it_says():
    """the control of the unequal plan from its definition: equally weighted window means on draw() average N / k^2 sum 1 / n_j"""
    windows = E.PLANS["unequal"][2]
    lw = E.law(50)
    m_j = E.window_sums(lw, E.rng_for(5), 1 << 14, windows) / np.asarray(windows, f64)[:, None]
    k = len(windows)
    wrong = ((m_j - m_j.mean(1, keepdims=True)) ** 2).sum(1) / (k * (k - 1))
    r, se = E.ratio(wrong / (lw.var / sum(windows)))
    want = E.control_equal_weights(windows)
    print(f"\n   equally weighted windows: {r} se {se}, expected {want:.4f}")
    assert abs(want - 1.7083333) < 1e-6 and (np.abs(r - want) <= E.Z_MAX * se).all()
    assert abs(E.control_equal_weights((64,) * 4) - 1.0) < 1e-15


def test_stopping_rule_on_draw():
    """64 fresh tiles under the header's rule against the 2048-tile simulation, per tile shape; k for k - 1 rejected for whole tiles;
    no stopping bias beyond the SE"""
    shapes = E.tile_shapes(44, 36)
    assert {s: int(m.sum()) for s, m in shapes.items()} == {(4, 4): 1, (4, 8): 4, (8, 4): 5, (8, 8): 20}
    assert {s: int(m.sum()) for s, m in E.tile_shapes(64, 64).items()} == {(8, 8): 64}
    fresh, _ = E.simulate_stopping(8, 8, tiles=64)
    rec = E.rule_c(fresh.reshape(8, 8), 64, 64, "draw()")[(8, 8)]
    print(f"\n   whole tiles: mean {rec[0]:.1f} over {rec[1]}, simulated {rec[2]:.1f}, se {rec[3]:.2f}, z {rec[4]:+.2f}, control z {rec[5]:+.2f}")
    for (tw, th) in shapes:
        count, bias = E.simulate_stopping(tw, th)
        ctl, _ = E.simulate_stopping(tw, th, divisor_k=True)
        b, bse = E.ratio(bias)
        print(f"   tiles of {tw} x {th}: {count.mean():.1f} +- {count.std(ddof=1):.1f} samples (k for k - 1: {ctl.mean():.1f}); frozen mean / mu - 1 "
              f"{np.round(b - 1, 5)} se {np.round(bse, 5)}")
        assert (count >= E.STOP["min_samples"]).all() and (count < E.STOP["budget"]).any()
        assert (np.abs(b - 1.0) <= E.Z_MAX * bse).all()


@pytest.mark.parametrize("D", E.ROBUST["depths"])
def test_robust_resolve_on_draw(D):
    """a 128 x 128 frame of draw() through the header's resolve steps, against the simulation of 20 times the pixels: MEAN meets rule A
    (k = K) and is unbiased; TRIM and GINI meet rule D; at max_depth 2 the unbiased value is rejected"""
    r, lw = E.ROBUST, E.law(D)
    m = E.robust_buckets(lw, E.rng_for(6, D), r["width"] * r["height"], r["K"], r["spp"])
    rgb, se, t = E.robust_resolve(m, E.MEAN)
    assert not t.any()
    a = E.rule_a(se, lw.var / r["spp"], 0.01, f"draw() MEAN D{D}", [(r["K"] - 1.0) / r["K"]])
    print(f"\n   MEAN D{D}: R {np.round(a[0], 4)} se {np.round(a[1], 4)} z {np.round(a[2], 2)} control z {np.round(a[3][0], 1)}")
    for mode, trim in ((E.TRIM, 1), (E.GINI, 0)):
        rgb, se, t = E.robust_resolve(m, mode, trim)
        b, bse, zb, v, vse, zv, sim = E.rule_d(rgb, se, D, mode, trim, f"draw() mode {mode} D{D}")
        print(f"   mode {mode} D{D}: rgb / mu {np.round(b, 4)} se {np.round(bse, 4)} z {np.round(zb, 2)} (simulated {np.round(sim[0], 4)} se "
              f"{np.round(sim[1], 5)}); stderr^2 N / sigma^2 {np.round(v, 4)} z {np.round(zv, 2)} (simulated {np.round(sim[2], 4)}); 2 t / j {sim[4]:.4f}")
        if D == 2:
            assert (np.abs(b - 1.0) > E.Z_MAX * bse).all()
        assert (np.abs(b - 1.0) <= sim[4] + E.Z_MAX * bse).all()


@pytest.mark.parametrize("D", E.ROBUST["depths"])
def test_host_build_of_robust_resolve_meets_rule_a(D, built):
    """vk_robust_resolve's own per-pixel code on the host (emu_robust_ffi) on a 64 x 64 frame of draw(): MEAN's stderr by rule A, TRIM and
    GINI by rule D"""
    import emu_robust_ffi
    r, lw = E.ROBUST, E.law(D)
    P, K, per = 64 * 64, r["K"], r["spp"] // r["K"]
    fixed = np.trunc(lw.table.astype(np.float32).astype(f64) * 2.0 ** 26).astype(np.int64)
    j = lw.draw_j(E.rng_for(7, D), (P, per, K))
    state = np.concatenate([fixed[j].sum(1), np.full((P, K, 1), per, np.int64)], -1)
    rgb, se = emu_robust_ffi.resolve(state, E.MEAN)
    a = E.rule_a(se, lw.var / r["spp"], 0.02, f"emu_robust MEAN D{D}", [(K - 1.0) / K])
    print(f"\n   host build, MEAN D{D}: R {np.round(a[0], 4)} se {np.round(a[1], 4)} z {np.round(a[2], 2)} control z {np.round(a[3][0], 1)}")
    for mode, trim in ((E.TRIM, 1), (E.GINI, 0)):
        rgb, se = emu_robust_ffi.resolve(state, mode, trim)
        b, bse, zb, v, vse, zv, sim = E.rule_d(rgb, se, D, mode, trim, f"emu_robust mode {mode} D{D}")
        print(f"   host build, mode {mode} D{D}: rgb / mu {np.round(b, 4)} z {np.round(zb, 2)}; stderr^2 N / sigma^2 {np.round(v, 4)} z {np.round(zv, 2)}")


@pytest.mark.parametrize("D", E.DEPTHS)
def test_temporal_rule_on_draw(D):
    """eight independent frames of draw() averaged as a fixed camera's history averages them (alpha = 1 / n: the running mean, the
    variances combined as those of independent frames): rule E after 1, 2, 4 and 8 frames, n - 1 for n rejected at n = 4"""
    t, lw = E.TEMPORAL, E.law(D)
    P = t["width"] * t["height"]
    color, var = np.zeros((P, 3)), np.zeros((P, 3))
    for frame in range(t["frames"]):
        mean, v = E.batch_means(E.window_sums(lw, E.rng_for(9, D, frame), P, t["windows"]), t["windows"])
        n = frame + 1
        k = 1.0 - 1.0 / n
        color, var = k * color + mean / n, k * k * var + v / (n * n)
        if n in t["checked"]:
            a, b = E.rule_e(color, np.sqrt(var), n, D, f"draw() D{D}", control=n - 1 if n == 4 else None)
            print(f"\n   D{D} n {n}: out_stderr3 R {np.round(a[0], 3)} se {np.round(a[1], 3)} z {np.round(a[2], 2)}; spread of out_color "
                  f"{np.round(b[0], 3)} se {np.round(b[1], 3)} z {np.round(b[2], 2)}" + (f" control z {np.round(b[3], 2)}" if b[3] is not None else ""), end="")
