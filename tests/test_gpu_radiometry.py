"""The integrators against closed-form radiometry, on the device, through the public ABI: vk_trace_radiance, vk_trace_irradiance and
vk_render on the cases of tests/radiometry_ref.py — the scenes, seeds, counts, expected values and power controls that
tests/test_radiometry.py holds the oracle and the emulator to.  A public call returns a mean per submitted record, so the same ray or
point is submitted 256 times (first_index gives each copy its own stream; a frame's 256 pixels are its replicas) and the rule is applied
to the replica means: |mean - want| <= 4 SE, SE <= 0.5 % of want, the power control rejected by |z| > 4.

These are the smallest shapes that still fill four waves and leave the public calls' per-record sample loops more than one chunk: 256
records, 16 x 16 frames, 256 to 2048 samples per record — at most 5 * 10^5 samples a case but for the glass ball at max_depth 2, whose
1.3 * 10^6 samples are two segments each (a sample is 1 with probability 0.04 there: fewer would leave SE above its cap)."""
import math

import numpy as np
import pytest

import radiometry_ref as R
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu
NAMES = list(R.STATISTICAL)


def device_means(ds, case):
    kw = dict(case.kw, samples_per_ray=case.spp)
    if case.route == "rays":
        got, st = ds.trace_radiance(case.items, return_stats=True, **kw)
    elif case.route == "points":
        got, st = ds.trace_irradiance(case.items, return_stats=True, **kw)
    else:
        return ds.render(case.cam, case.render_params())[0]
    assert st.samples == len(case.items) * case.spp and st.kernel_ms > 0
    return got


def report(name, results):
    for g, (mean, se, z) in enumerate(results):
        print(f"\n   {name}[{g}]: mean {np.round(mean, 6)} se {np.round(se, 6)} z {np.round(z, 2)}", end="")


@pytest.mark.parametrize("name", NAMES)
def test_public_call_meets_the_closed_form(name, device):
    case = R.STATISTICAL[name]()
    owner, desc = case.scene()
    ds = DeviceScene(desc)
    try:
        # what the world is walked on.  A tree of fewer than 16 objects is kept as handed over whatever the flags; the 18 spheres of the
        # `tops` world are rebuilt by default (exact re-treeing) and under VK_SCENE_FAST_ACCEL; the integrating sphere's crowd variant
        # under VK_SCENE_FAST_ACCEL (what its default takes is the lineariser's choice: printed, not asserted)
        tree = ds.info().tree
        print(f"\n   flags {case.flags}: tree {tree}", end="")
        if case.flags == ffi.VK_SCENE_REFERENCE_TREE:
            assert tree == ffi.VK_TREE_HANDED_OVER
        elif name in ("sphere-crowd-frame-D3-fast-accel", "tops-D50-fast-accel"):
            assert tree == ffi.VK_TREE_REBUILT_FAST
        elif name.startswith("tops"):
            assert tree in (ffi.VK_TREE_REBUILT_PROVEN, ffi.VK_TREE_REBUILT_NEAR, ffi.VK_TREE_REBUILT_GRID)
        elif name != "sphere-crowd-frame-D3":
            assert tree == ffi.VK_TREE_HANDED_OVER
        report(name, case.check_means(device_means(ds, case), "device"))
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["rect-rays-D50-pdf", "rect-rays-two-lights", "sphere-irradiance-D3", "glass-D4-scatter", "fog-pdf"])
def test_per_sample_hooks_meet_the_closed_form(name, device):
    """the per-sample route of the device (vk_debug_trace_radiance_samples / vk_debug_trace_irradiance_samples): SE from the samples"""
    case = R.STATISTICAL[name]()
    owner, desc = case.scene()
    ds = DeviceScene(desc)
    try:
        kw = dict(case.kw, samples_per_ray=case.spp)
        samples = ds.debug_radiance_samples(case.items, **kw) if case.route == "rays" else ds.debug_irradiance_samples(case.items, **kw)[0]
        report(name, case.check_samples(samples, "device hook"))
    finally:
        ds.close()


def test_regenerating_run_with_roulette_keeps_the_closed_form(device):
    """the integrating sphere's frame at max_depth 50 through Film.render_regen with vk_roulette_set on: the rule is unbiased, so the
    closed form survives it.  SE / want from the pixels' spread: 0.32 % / 0.24 % / 0.20 % expected (a simulation of the rule (2, 0.1, 0.8)
    on this scene's Markov chain in f64 numpy, 262 144 paths; 0.28 % / 0.19 % / 0.09 % without the rule)."""
    case = R.sphere_frame(50)
    owner, desc = case.scene()
    ds = DeviceScene(desc)
    try:
        p = case.render_params()
        plain, _ = ds.render(case.cam, p)
        with ds.film(case.cam, p) as film, ds.paths(4096) as pb:
            img = film.render_regen(pb, roulette=(2, 0.1, 0.8))
            assert pb.roulette() is not None and pb.info().retired[ffi.VK_PATHS_CULLED] > 0
        assert not np.array_equal(img, plain)
        report(case.name + " regen + roulette", case.check_means(img, "device, regenerating run with roulette"))
    finally:
        ds.close()


@pytest.mark.parametrize("integrator", [R.PDF, R.SCATTER], ids=["pdf", "scatter"])
def test_mirror_is_exact(integrator, device):
    case = R.mirror(integrator)
    owner, desc = case.scene()
    ds = DeviceScene(desc)
    try:
        kw = dict(case.kw, samples_per_ray=case.spp)
        dev_m = R.mirror_deviation(ds.trace_radiance(case.items, **kw))
        dev_s = R.mirror_deviation(ds.debug_radiance_samples(case.items, **kw))
        print(f"\n   largest relative deviation from f64: means {dev_m:.2e}, samples {dev_s:.2e}")
        assert dev_m <= R.MIRROR_TOL and dev_s <= R.MIRROR_TOL
    finally:
        ds.close()


def test_a_sphere_in_lights_biases_the_pdf_integrator(device):
    """property A (radiometry_ref.property_a): blue sits ABOVE the radiometric value by z > 4, as the reference's does"""
    case = R.property_a()
    owner, desc = case.scene()
    ds = DeviceScene(desc)
    try:
        mean, se, z = R.z_scores(device_means(ds, case), case.want[0])
        print(f"\n   mean / radiometric - 1 = {np.round(mean / case.want[0] - 1, 4)}, z {np.round(z, 2)}")
        assert (se <= R.SE_CAP * case.want[0]).all()
        assert z[2] > R.Z_MAX
    finally:
        ds.close()


def test_a_flipped_entry_in_lights_drops_half_of_the_samples(device):
    """property B (radiometry_ref.property_b): the public call's mean meets the closed form; on the hook half of the samples are NaN"""
    case = R.property_b()
    owner, desc = case.scene()
    ds = DeviceScene(desc)
    try:
        report(case.name, case.check_means(device_means(ds, case), "device"))
        x = ds.debug_radiance_samples(case.items, **dict(case.kw, samples_per_ray=case.spp))[..., :3].reshape(-1, 3)
        n, dropped = len(x), R.clean(x)[1]
        print(f"\n   {dropped} of {n} samples dropped")
        assert abs(dropped / n - 0.5) <= R.Z_MAX * 0.5 / math.sqrt(n)
    finally:
        ds.close()
