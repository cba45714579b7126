"""The error estimates and stopping rules on the device, through the public calls, against a known sample law.

vk_progress_stderr, vk_adapt_stderr, the tile decisions of vk_progress_set_adaptive and vk_adapt_*, vk_robust_resolve's stderr3 and
vk_temporal_accumulate's out_stderr3 are elsewhere compared bit for bit with numpy restatements of their formulas.  Here they are held
to what the header says they MEAN, on the integrating sphere's frame, whose every pixel is an independent draw from a law known in closed
form (tests/estimator_laws_ref.py: the law, the rules A to E, their power controls, the f64 simulations on numpy's own generator).  No
restatement module takes part.

Shapes: 32 x 32 to 128 x 128 pixels, 16 to 1024 samples per pixel, at most 4 * 10^6 samples a case."""
import numpy as np
import pytest

import estimator_laws_ref as E
import radiometry_ref as R
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ds(device):
    owner, desc = R.sphere_scene()
    scene = DeviceScene(desc)
    yield scene
    scene.close()


def sphere_params(w, h, spp, D, seed=E.SEED):
    return R.params(w, h, spp, max_depth=D, seed=seed, integrator=R.SCATTER)


def progressive(ds, w, h, windows, D, seed=E.SEED):
    """(mean, stderr) of the frame accumulated over the windows by vk_progress"""
    with ds.progress(R.sphere_camera(), sphere_params(w, h, sum(windows), D, seed), stderr=True) as pr:
        for n in windows:
            img, _ = pr.step(n)
        assert pr.info().clamped_samples == 0
        return img.copy(), pr.stderr()


def through_film(ds, w, h, windows, D):
    """the same frame through a film's error moments: tolerances 0 (no tile ever freezes), tile runs through a 4096-slot batch"""
    with ds.film(R.sphere_camera(), sphere_params(w, h, sum(windows), D)) as film, ds.paths(4096) as pb:
        film.enable_adaptive(abs_tol=0.0, rel_tol=0.0)
        if len(set(windows)) == 1:
            img, info = film.render_adaptive(pb, windows[0])
        else:
            for n in windows:
                film.adapt_begin(pb, n)
                while True:
                    r = film.regen_step(pb, 0xFFFFFFFF)
                    if r.live == 0 and r.remaining == 0:
                        break
                info = film.adapt_close(n)
            img = film.resolve_adaptive()
        assert info.samples_done == sum(windows) and info.steps == len(windows) and info.tiles_active == info.tiles_total
        return img, film.stderr()


def controls_a(plan):
    windows = E.PLANS[plan][2]
    return [E.control_divisor_k(windows)] + ([E.control_equal_weights(windows)] if len(set(windows)) > 1 else [])


def show(what, *figures):
    print(f"\n   {what}: " + "  ".join(str(np.round(np.asarray(f, float), 4)) for f in figures), end="")


# ---------------------------------------------------------------- A and B: vk_progress_stderr and vk_adapt_stderr
@pytest.mark.parametrize("D", E.DEPTHS)
@pytest.mark.parametrize("plan", list(E.PLANS))
def test_batch_means_variance_and_coverage(plan, D, ds):
    """rule A: the mean over pixels of stderr^2 / (sigma^2 / N) is 1; the divisor k and, for unequal windows, equally weighted window
    means are rejected.  Rule B: the error bars cover mu as often as the same plan does on draw()."""
    w, h, windows, cap = E.PLANS[plan]
    lw = E.law(D)
    mean, se = progressive(ds, w, h, windows, D)
    assert np.isfinite(mean).all() and np.isfinite(se).all() and (se >= 0).all()
    r, rse, z, zc = E.rule_a(se, lw.var / sum(windows), cap, f"vk_progress_stderr {plan} D{D}", controls_a(plan))
    show(f"A {plan} D{D}", r, rse, z, *zc)
    got, want, zb, ctrl, zbc, asked = E.rule_b(mean, se, D, plan, f"vk_progress_stderr {plan} D{D}")
    show(f"B {plan} D{D}", got, want, zb, ctrl, zbc, asked)
    if plan in ("k2", "equal64", "k8_128"):
        assert asked.any(), "the run that exists to reject rule B's control does not ask for it"


@pytest.mark.parametrize("D", E.DEPTHS)
@pytest.mark.parametrize("plan", ["equal", "unequal", "k2"])
def test_film_moments_variance_and_coverage(plan, D, ds):
    """the same rules for Film.stderr (vk_adapt_stderr) of the frame carried by tile runs through a 4096-slot path batch"""
    w, h, windows, cap = E.PLANS[plan]
    lw = E.law(D)
    mean, se = through_film(ds, w, h, windows, D)
    r, rse, z, zc = E.rule_a(se, lw.var / sum(windows), cap, f"vk_adapt_stderr {plan} D{D}", controls_a(plan))
    show(f"A film {plan} D{D}", r, rse, z, *zc)
    got, want, zb, ctrl, zbc, asked = E.rule_b(mean, se, D, plan, f"vk_adapt_stderr {plan} D{D}")
    show(f"B film {plan} D{D}", got, want, zb, ctrl, zbc, asked)


# ---------------------------------------------------------------- C: the stopping rule
def adaptive_kw():
    s = E.STOP
    return dict(abs_tol=s["abs_tol"], rel_tol=s["rel_tol"], min_samples=s["min_samples"], min_steps=s["min_steps"])


def check_stopped(what, w, h, img, se, tiles):
    s = E.STOP
    assert (tiles >= s["min_samples"]).all() and (tiles <= s["budget"]).all() and (tiles % s["window"] == 0).all()
    for shape, rec in E.rule_c(tiles, w, h, what).items():
        show(f"C {what} {w}x{h} tiles {shape}", *rec)
    worst, frozen = E.frozen_within_tolerance(img, se, tiles, w, h)
    show(f"C {what} {w}x{h} frozen tiles, worst stderr / tolerance", frozen, worst)
    assert frozen > 0 and worst <= 1.0 + 1e-6
    for mean, mse, z in E.stop_case(w, h).check_means(img, what):
        show(f"C {what} {w}x{h} frozen frame / closed form", mean, mse, z)


@pytest.mark.parametrize("w,h", [(64, 64), (44, 36)])
def test_stopping_rule_progress(w, h, ds):
    """the tiles of an adaptive vk_progress stop where the header's rule stops them on draw(): the mean tile count per tile shape (the
    44 x 36 frame has tiles of 4 x 8, 8 x 4 and 4 x 4 in-image pixels), the control k for k - 1 rejected, the frozen frame still the
    closed form, every frozen pixel within the tolerance that stopped it"""
    s = E.STOP
    with ds.progress(R.sphere_camera(), sphere_params(w, h, s["budget"], s["D"]), adaptive=adaptive_kw()) as pr:
        img = None
        for _ in range(s["budget"] // s["window"]):
            img, _ = pr.step(s["window"])
            if pr.tile_samples()[1].tiles_active == 0:
                break
        tiles, inf = pr.tile_samples()
        se = pr.stderr()
        assert pr.info().clamped_samples == 0
    assert inf.samples_rendered < w * h * s["budget"]
    check_stopped("vk_progress", w, h, img, se, tiles)


@pytest.mark.parametrize("w,h", [(64, 64), (44, 36)])
def test_stopping_rule_film(w, h, ds):
    """the same plan through Film.render_adaptive (vk_adapt_*)"""
    s = E.STOP
    with ds.film(R.sphere_camera(), sphere_params(w, h, s["budget"], s["D"])) as film, ds.paths(1 << 16) as pb:
        film.enable_adaptive(**adaptive_kw())
        img, info = film.render_adaptive(pb, s["window"])
        tiles, inf = film.tile_samples()
        se = film.stderr()
    check_stopped("vk_adapt", w, h, img, se, tiles)


# ---------------------------------------------------------------- D: the robust film
@pytest.fixture(scope="module", params=E.ROBUST["depths"])
def robust_frame(request, ds):
    """(D, {mode: (rgb, stderr3)}) of one 128 x 128 x 64 spp frame deposited into K = 8 buckets by Robust.render"""
    D, r = request.param, E.ROBUST
    with ds.film(R.sphere_camera(), sphere_params(r["width"], r["height"], r["spp"], D)) as film, ds.paths(1 << 18) as pb, \
            ds.robust(r["width"], r["height"], r["spp"], buckets=r["K"], mode=ffi.VK_ROBUST_MEAN) as rb:
        rb.render(film, pb)
        inf = rb.info()
        assert inf.deposited == r["width"] * r["height"] * r["spp"] and inf.dropped == 0 and inf.clamped == 0
        return D, {mode: rb.resolve(mode=mode, trim=trim, want_stderr=True)
                   for mode, trim in ((ffi.VK_ROBUST_MEAN, 0), (ffi.VK_ROBUST_TRIM, 1), (ffi.VK_ROBUST_GINI, 0))}


def test_robust_mean_stderr_is_the_standard_error(robust_frame):
    """MEAN: stderr3^2 against sigma^2 / N by rule A with k = K, the divisor K rejected; the frame itself unbiased"""
    D, frames = robust_frame
    lw, r = E.law(D), E.ROBUST
    rgb, se = frames[ffi.VK_ROBUST_MEAN]
    a = E.rule_a(se, lw.var / r["spp"], 0.01, f"vk_robust_resolve MEAN D{D}", [(r["K"] - 1.0) / r["K"]])
    show(f"D MEAN D{D} stderr", *a[:3], *a[3])
    b, bse = E.ratio(rgb.astype(np.float64).reshape(-1, 3) / lw.mu)
    show(f"D MEAN D{D} rgb / mu", b, bse, (b - 1) / bse)
    assert (np.abs(b - 1.0) <= E.Z_MAX * bse).all()


@pytest.mark.parametrize("mode,trim", [(ffi.VK_ROBUST_TRIM, 1), (ffi.VK_ROBUST_GINI, 0)], ids=["trim1", "gini"])
def test_robust_trimmed_means_against_the_simulation(mode, trim, robust_frame):
    """TRIM and GINI: the frame's mean of rgb / mu and of stderr^2 N / sigma^2 against the header's seven resolve steps on draw(); at
    max_depth 2 (a sample is a Le or 0) the unbiased value 1 is rejected; the bias stays within the trimmed share 2 t / j"""
    D, frames = robust_frame
    rgb, se = frames[mode]
    b, bse, zb, v, vse, zv, sim = E.rule_d(rgb, se, D, mode, trim, f"vk_robust_resolve mode {mode} D{D}")
    show(f"D mode {mode} D{D} rgb / mu", b, bse, zb, sim[0], sim[1])
    show(f"D mode {mode} D{D} stderr^2 N / sigma^2", v, vse, zv, sim[2], sim[3])
    if D == 2:
        z1 = (b - 1.0) / bse
        show(f"D mode {mode} D{D} z against the unbiased value", z1)
        assert (np.abs(z1) > E.Z_MAX).all(), f"the unbiased value 1 is not rejected: {b} se {bse}"
    show(f"D mode {mode} D{D} trimmed share 2 t / j", sim[4])
    assert (np.abs(b - 1.0) <= sim[4] + E.Z_MAX * bse).all(), f"bias {b - 1} beyond the trimmed share {sim[4]}"


# ---------------------------------------------------------------- E: temporal accumulation at a fixed camera
@pytest.mark.parametrize("D", E.DEPTHS)
def test_temporal_variance_at_a_fixed_camera(D, ds):
    """eight frames of neighbouring seeds, each with its own vk_progress_stderr and first-hit buffers, blended at a fixed camera: after
    n = 1, 2, 4, 8 frames out_stderr3^2 averages sigma^2 / (64 n) and the pixels' spread of out_color is that too (frames of
    neighbouring seeds are independent); n - 1 for n is rejected at n = 4"""
    t = E.TEMPORAL
    w, h, cam = t["width"], t["height"], R.sphere_camera()
    with ds.temporal(w, h, max_history=16) as acc:
        for frame in range(t["frames"]):
            seed = E.frame_seed(frame)
            color, se = progressive(ds, w, h, t["windows"], D, seed)
            aov, _ = ds.render_aov(cam, sphere_params(w, h, sum(t["windows"]), D, seed))
            out, out_se, hist, _ = acc.accumulate(cam, color, aov["normal"], aov["depth"], stderr=se, albedo=aov["albedo"], want_history=True)
            n = frame + 1
            # (the history length is a bilinear blend of taps that all hold n - 1: n to f32 rounding)
            assert (np.abs(hist - n) <= n * 2.0 ** -22).all(), f"frame {frame}: history {np.unique(hist)}"
            if n in t["checked"]:
                a, b = E.rule_e(out, out_se, n, D, f"vk_temporal_accumulate D{D}", control=n - 1 if n == 4 else None)
                show(f"E D{D} n {n} out_stderr3", *a[:3], *a[3])
                show(f"E D{D} n {n} spread of out_color", *[x for x in b if x is not None])
