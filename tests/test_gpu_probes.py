"""Probe queries on the device: vk_trace_probes and its per-sample hook.  The hook's directions against the replay of tests/probes_ref.py
and its samples against vk_debug_trace_radiance_samples on the replayed rays and resumed streams, on the scenes of tests/test_rays_emu.py;
the public call against the hook by the fixed-point rule (tests/exact_sums.py) over a sample's 27 products; probe order, batch cuts, sample
windows and staged chunks bit for bit; the direction field unread; degenerate cases.  Every comparison is exact (a NaN's payload aside)
but the closed form's, the one check that shares no restatement with the code."""
import numpy as np
import pytest

import probes_ref as ref
import test_rays_emu as shared
from vecchio_amd import DeviceScene, ffi
from vecchio_amd.scene import make_points, make_probes, probe_eval

pytestmark = pytest.mark.gpu
f32 = np.float32
bits = ref.bits
THREE = ["final_scene", "cornell_box", "random_spheres_iow"]      # everything with media, Cornell-type, spheres only


def kwargs(hs, **over):
    kw = dict(seed=41, first_index=1000, samples_per_ray=1, first_sample=0, max_depth=12, integrator=hs.integrator,
              background=hs.background, background_color=hs.background_color)
    kw.update(over)
    return kw


def scene_probes(oracle, hs, cam, n):
    lo, hi = ref.scene_box(oracle, hs.desc, cam, hs.params(20, 1, 50, height=12))
    return ref.probes_in_box(n, lo, hi, float(cam.time0), float(cam.time1))


# ---------------------------------------------------------------- against the radiance query's device path
@pytest.mark.parametrize("kind,name", shared.SCENES, ids=[f"{k}-{n}" for k, n in shared.SCENES])
def test_scene_against_the_radiance_querys_samples(kind, name, device, oracle, host_scenes):
    n, spp = 9, 5
    owner, desc, cam, p = ref.scene(kind, name, host_scenes)
    lo, hi = ref.scene_box(oracle, desc, cam, p)
    probes = ref.probes_in_box(n, lo, hi, float(cam.time0), float(cam.time1))
    ds = DeviceScene(desc)
    try:
        for integ in ref.integrators_allowed(desc, p.integrator):
            kw = ref.params_kwargs(p, seed=p.seed + 23, first_index=2 ** 40 + 5, samples_per_ray=spp, max_depth=50, integrator=integ)
            samples, dirs, st = ds.debug_probe_samples(probes, return_stats=True, **kw)
            assert st.samples == n * spp and st.kernel_launches == 1 and st.kernel_ms > 0
            rdirs, keys = ref.directions(oracle, probes, **kw)
            ref.assert_same_floats(dirs[..., :3], rdirs, f"{kind} {name} integrator {integ}: directions")
            assert not bits(dirs[..., 3]).any()
            want = ds.debug_radiance_samples(ref.replayed_rays(probes, rdirs), keys.reshape(-1),
                                             **dict(kw, samples_per_ray=1, first_sample=0, first_index=0))
            ref.assert_same_samples(samples, want.reshape(n, spp, 4), f"{kind} {name} integrator {integ}: samples")
            assert (bits(samples[..., 3]) >= keys["ctr"]).all() and keys["ctr"].min() >= 3
            # the public call is the exact fixed-point mean of the hook's (L, u)
            sh, clamped, _ = ref.exact_probes(samples, dirs)
            got, st = ds.trace_probes(probes, return_stats=True, **kw)
            np.testing.assert_array_equal(bits(got), bits(sh), err_msg=f"{kind} {name} integrator {integ}")
            assert st.samples == n * spp and st.clamped_samples == clamped
    finally:
        ds.close()


# ---------------------------------------------------------------- one value per index
@pytest.mark.parametrize("name", THREE)
def test_one_value_per_index(name, device, oracle, host_scenes):
    """n below, at and across the 8-probe unit and across what would be a 64-slot boundary; 1 sample, a few, and 64 (with few probes:
    16 sample chunks a unit, so several waves add to one probe).  The public call against the hook's exact mean; permuted probes at their
    own indices; the batch cut at 3 and at 8; two sample windows, each the exact mean of its rows of the whole window's samples (their
    integer sums add up to the whole window's)"""
    hs, cam = host_scenes(name)
    ds = DeviceScene(hs.desc)
    try:
        all_probes = scene_probes(oracle, hs, cam, 130)
        for n in (1, 7, 8, 9, 64, 65, 130):
            probes = all_probes[:n]
            for spp in (1, 5, 64):
                what = f"{name} n {n} spp {spp}"
                kw = kwargs(hs, samples_per_ray=spp)
                samples, dirs = ds.debug_probe_samples(probes, **kw)
                want, clamped, sums = ref.exact_probes(samples, dirs)
                got, st = ds.trace_probes(probes, return_stats=True, **kw)
                np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)
                assert st.samples == n * spp and st.kernel_launches == 1 and st.clamped_samples == clamped and np.isfinite(got).all()
                # each probe alone at its own index, in a permuted order (a few of them)
                for j in np.random.default_rng(n * 100 + spp).permutation(n)[:4]:
                    one = ds.trace_probes(probes[j:j + 1], **dict(kw, first_index=kw["first_index"] + int(j)))
                    np.testing.assert_array_equal(bits(one[0]), bits(got[j]), err_msg=f"{what} probe {j}")
                for cut in (3, 8):
                    if cut < n:
                        parts = [ds.trace_probes(probes[lo:hi], **dict(kw, first_index=kw["first_index"] + lo))
                                 for lo, hi in ((0, cut), (cut, n))]
                        np.testing.assert_array_equal(bits(np.concatenate(parts)), bits(got), err_msg=f"{what} cut {cut}")
                if spp > 1:
                    a = 3
                    total = np.zeros_like(sums)
                    for first, count in ((0, a), (a, spp - a)):
                        wkw = dict(kw, first_sample=first, samples_per_ray=count)
                        wsamples, wdirs = ds.debug_probe_samples(probes, **wkw)
                        ref.assert_same_samples(wsamples, samples[:, first:first + count], f"{what} window {first}")
                        ref.assert_same_floats(wdirs, dirs[:, first:first + count], f"{what} window {first}")
                        wwant, _, wsums = ref.exact_probes(wsamples, wdirs)
                        np.testing.assert_array_equal(bits(ds.trace_probes(probes, **wkw)), bits(wwant), err_msg=f"{what} window {first}")
                        total += wsums
                    if clamped == 0:
                        np.testing.assert_array_equal(total, sums)
    finally:
        ds.close()


def test_the_direction_field_is_not_read(device, oracle, host_scenes):
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    try:
        probes = scene_probes(oracle, hs, cam, 21)
        kw = kwargs(hs, samples_per_ray=6)
        want = ds.trace_probes(probes, **kw)
        wsamples, wdirs = ds.debug_probe_samples(probes, **kw)
        for d in (np.nan, 0.0, np.inf, None):
            other = probes.copy()
            other["direction"] = np.random.default_rng(3).normal(size=(21, 3)).astype(f32) * 1e6 if d is None else d
            np.testing.assert_array_equal(bits(ds.trace_probes(other, **kw)), bits(want), err_msg=str(d))
            s, u = ds.debug_probe_samples(other, **kw)
            np.testing.assert_array_equal(bits(s), bits(wsamples)), np.testing.assert_array_equal(bits(u), bits(wdirs))
    finally:
        ds.close()


def test_the_host_call_works_in_chunks(device, oracle, host_scenes):
    """more probes than the staging buffer holds (2^20): two launches, and first_index makes the cut invisible; the per-sample hook
    stages 2^22 samples at a time: at 2^21 samples per probe three probes are two launches (2 + 1) that cut an 8-probe unit"""
    hs, cam = host_scenes("random_spheres_iow")
    n = (1 << 20) + 13
    ds = DeviceScene(hs.desc)
    try:
        probes = np.resize(scene_probes(oracle, hs, cam, 4096), n)
        kw = kwargs(hs, first_index=2 ** 40, max_depth=3)
        got, st = ds.trace_probes(probes, return_stats=True, **kw)
        assert st.kernel_launches == 2 and st.samples == n
        tail = ds.trace_probes(probes[-21:], **dict(kw, first_index=2 ** 40 + n - 21))
        np.testing.assert_array_equal(bits(got[-21:]), bits(tail))
        assert (got[:4096] != got[4096:8192]).any()       # the same probe at another index draws from another stream
        kw = kwargs(hs, first_index=2 ** 40, max_depth=2, samples_per_ray=1 << 21)
        samples, dirs, st = ds.debug_probe_samples(probes[:3], return_stats=True, **kw)
        assert st.kernel_launches == 2 and st.samples == 3 << 21
        for i in range(3):
            s1, d1 = ds.debug_probe_samples(probes[i:i + 1], **dict(kw, first_index=2 ** 40 + i))
            np.testing.assert_array_equal(bits(samples[i]), bits(s1[0]), err_msg=f"probe {i}")
            np.testing.assert_array_equal(bits(dirs[i]), bits(d1[0]), err_msg=f"probe {i}")
    finally:
        ds.close()


# ---------------------------------------------------------------- the closed form
SKY = dict(seed=2024, first_index=7, samples_per_ray=16384, max_depth=50, integrator=ffi.VK_INTEGRATOR_SCATTER,
           background=ffi.VK_BACKGROUND_SKY)


def test_the_skys_closed_form(device, host_scenes):
    """4 probes with tmax = 0: no walk runs, every sample is the sky a_c + b_c * y along u.  E[sh_0,c] = a_c * 0.282095, E[sh_1,c] = b_c *
    0.488603 / 3, every other coefficient 0; 16384 samples, every product within +-1.1: by Hoeffding each of the 108 values leaves the
    band of 0.05 with probability 2 exp(-2 * 16384 * 0.05^2 / 2.2^2) = 9e-8, all of them below 1e-5.
    tests/test_probes_emu.py runs the same inputs through the emulator."""
    hs, cam = host_scenes("random_spheres_iow")
    ds = DeviceScene(hs.desc)
    try:
        probes = make_probes(np.zeros((4, 3), f32), tmax=0.0)
        sh, st = ds.trace_probes(probes, return_stats=True, **SKY)
        err = np.abs(sh - ref.sky_expected()[None])
        print(f"\n   max |sh - E[sh]| over 4 x 27 values: {err.max():.4f}")
        assert st.samples == 4 * 16384 and st.clamped_samples == 0
        assert (err <= 0.05).all(), err.max()
        assert (bits(sh[0]) != bits(sh[1])).any()
        # vk_probe_eval mode 1 on the result against vk_trace_irradiance at the same place: both estimate irradiance / pi, the probe
        # within eval_band(0.05) and the gather — a mean of 16384 values in [0, 1] — within 0.05 by the same bound
        for nrm in ([0, 1, 0], [0, -1, 0], [1, 0, 0], [0.3, 0.5, -0.2]):
            irr = ds.trace_irradiance(make_points(np.zeros((1, 3), f32), [nrm], tmax=0.0), **SKY)[0]
            ev = probe_eval(sh[0], nrm, 1)
            band = ref.eval_band(nrm, 1, 0.05) + 0.05
            print(f"   normal {nrm}: probe_eval {ev}, trace_irradiance {irr}, band {band:.3f}")
            assert (np.abs(ev - irr) <= band).all(), (nrm, ev, irr)
    finally:
        ds.close()


# ---------------------------------------------------------------- degenerate cases
def test_max_depth_zero_and_no_probes(device, oracle, host_scenes):
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    try:
        probes = scene_probes(oracle, hs, cam, 11)
        kw = kwargs(hs, samples_per_ray=4, max_depth=0)
        out = np.full((11, 9, 3), 7.0, f32)
        got, st = ds.trace_probes(probes, out=out, return_stats=True, **kw)
        assert not bits(got).any() and st.samples == 44 and st.kernel_launches == 0
        zero, zdirs = ds.debug_probe_samples(probes, **kw)
        assert not bits(zero).any() and not bits(zdirs).any()
        got, st = ds.trace_probes(probes[:0], return_stats=True, **kwargs(hs, samples_per_ray=4))
        assert got.shape == (0, 9, 3) and st.samples == 0 and st.kernel_launches == 0
    finally:
        ds.close()


def test_clamped_samples_in_front_of_a_hot_emitter(device):
    """a light of radiance 4e10 (tests/test_gpu_abi2.py's firefly scene): a sample that sees it has products beyond the clamp of 1e10,
    saturates and counts once, whichever of its 27 products were clamped"""
    from descs import Desc
    d = Desc()
    hot = d.light(4e10, 4e10, 4e10)
    q = d.xy_rect(-1.0, 1.0, -1.0, 1.0, 0.0, hot)
    grey = d.sphere((0.0, -101.0, 0.0), 100.0, d.lambertian(0.5, 0.5, 0.5))
    desc = d.finish(d.big_box(q, grey), [q])
    ds = DeviceScene(desc)
    try:
        probes = make_probes([[0, 0, 0.5], [0, 0, -0.5], [0.3, 0.2, 0.25], [-0.3, 0.1, -0.25]])
        kw = dict(seed=5, first_index=0, samples_per_ray=12, max_depth=4, integrator=ffi.VK_INTEGRATOR_SCATTER,
                  background=ffi.VK_BACKGROUND_SOLID, background_color=(0.1, 0.1, 0.1))
        samples, dirs = ds.debug_probe_samples(probes, **kw)
        want, clamped, _ = ref.exact_probes(samples, dirs)
        got, st = ds.trace_probes(probes, return_stats=True, **kw)
        np.testing.assert_array_equal(bits(got), bits(want))
        assert clamped > 0 and st.clamped_samples == clamped and np.isfinite(got).all()
        assert np.abs(got).max() > 1e8
    finally:
        ds.close()
