"""Probe queries on the CPU: vk_trace.h probe_sample and sh9 (through tests/emu/emu_probes.cpp) against the chain of tests/probes_ref.py —
the oracle's gen_range(-1, 1) draws, a numpy replay of random_in_unit_sphere and unit_vector, then the radiance query's per-sample path
(radiance_sample through tests/emu/emu_radiance.cpp, which tests/test_radiance_emu.py holds to the oracle) on the replayed ray with the
stream resumed behind the direction's 3 * tries draws — and the basis against its numpy restatement.  Every comparison is bit for bit (a
NaN's payload aside) but the closed form's.  67 probes x 4 samples per scene and integrator; tests/test_gpu_probes.py runs the chain on
the device."""
import numpy as np
import pytest

import probes_ref as ref
import special_scenes
from test_emu_parity import BUILDER_SCENES
from vecchio_amd import ffi
from vecchio_amd.scene import make_probes, probe_eval

f32 = np.float32
N, SPP = 67, 4


@pytest.fixture(scope="session")
def emu_probes(built):
    import emu_probes_ffi
    emu_probes_ffi.load()
    return emu_probes_ffi


@pytest.fixture(scope="session")
def emu_radiance(built):
    import emu_radiance_ffi
    emu_radiance_ffi.load()
    return emu_radiance_ffi


def through_the_radiance_path(oracle, emu_radiance, desc, probes, kw):
    """(replayed directions, their keys, the samples the radiance path gives for them): kw's window of every probe"""
    rdirs, keys = ref.directions(oracle, probes, **kw)
    want, _ = emu_radiance.radiance_samples(desc, ref.replayed_rays(probes, rdirs), keys.reshape(-1),
                                            **dict(kw, samples_per_ray=1, first_sample=0, first_index=0))
    return rdirs, keys, want.reshape(len(probes), kw["samples_per_ray"], 4)


def run_chain(oracle, emu_probes, emu_radiance, desc, cam, p, what):
    lo, hi = ref.scene_box(oracle, desc, cam, p)
    probes = ref.probes_in_box(N, lo, hi, float(cam.time0), float(cam.time1))
    for integ in ref.integrators_allowed(desc, p.integrator):
        kw = ref.params_kwargs(p, seed=p.seed + 23, first_index=2 ** 40 + 5, samples_per_ray=SPP, max_depth=50, integrator=integ)
        samples, dirs, basis = emu_probes.probe_samples(desc, probes, **kw)
        # (a) the directions are the replay's, unit length; (b) the samples are the radiance path's on the replayed rays and resumed
        # streams; (c) the basis is the numpy restatement's
        rdirs, keys, want = through_the_radiance_path(oracle, emu_radiance, desc, probes, kw)
        ref.assert_same_floats(dirs[..., :3], rdirs, f"{what} integrator {integ}: directions")
        assert not ref.bits(dirs[..., 3]).any() and np.isfinite(dirs).all()
        np.testing.assert_allclose(np.linalg.norm(dirs[..., :3].astype(np.float64), axis=-1), 1.0, atol=1e-6)
        ref.assert_same_samples(samples, want, f"{what} integrator {integ}: samples")
        ref.assert_same_floats(basis, ref.sh9(rdirs), f"{what} integrator {integ}: basis")
        ctr = ref.bits(samples[..., 3])
        assert (ctr >= keys["ctr"]).all() and (keys["ctr"] % 3 == 0).all() and keys["ctr"].min() == 3 and keys["ctr"].max() > 3
        # a probe whose first segment is not walked sees the background at once: its stream stands behind the direction's draws
        for i in range(0, N, 3):
            if not probes["tmax"][i] > 0.001:
                assert (ctr[i] == keys["ctr"][i]).all(), i
        # (d) `direction` is not read
        other = probes.copy()
        other["direction"] = f32([1, 2, 3])
        s2, d2, _ = emu_probes.probe_samples(desc, other, **kw)
        ref.assert_same_samples(s2, samples, f"{what}: direction"), ref.assert_same_floats(d2, dirs, f"{what}: direction")
        # (e) the window [3, 8) is rows 3..7 of the window [0, 8)
        full, fdirs, _ = emu_probes.probe_samples(desc, probes, **dict(kw, samples_per_ray=8))
        win, wdirs, _ = emu_probes.probe_samples(desc, probes, **dict(kw, samples_per_ray=5, first_sample=3))
        ref.assert_same_samples(win, full[:, 3:8], f"{what} integrator {integ}: window")
        ref.assert_same_floats(wdirs, fdirs[:, 3:8], f"{what} integrator {integ}: window directions")
        ref.assert_same_samples(full[:, :SPP], samples, f"{what} integrator {integ}: the first rows of a longer window")
        # (f) max_depth 0: (0,0,0) without a draw
        zero, zdirs, zb = emu_probes.probe_samples(desc, probes, **dict(kw, max_depth=0))
        assert not ref.bits(zero).any() and not ref.bits(zdirs).any() and not ref.bits(zb).any()


@pytest.mark.parametrize("name", BUILDER_SCENES)
def test_builder_scene(name, oracle, emu_probes, emu_radiance, host_scenes):
    hs, cam = host_scenes(name)
    run_chain(oracle, emu_probes, emu_radiance, hs.desc, cam, hs.params(20, 1, 50, height=12), name)


@pytest.mark.parametrize("name", sorted(special_scenes.ALL))
def test_special_scene(name, oracle, emu_probes, emu_radiance, built):
    d, desc, cam, p = special_scenes.ALL[name]()
    run_chain(oracle, emu_probes, emu_radiance, desc, cam, p, name)


def test_the_replay_against_closed_forms(oracle):
    """the numpy restatement itself: the rejection loop on hand-made draws, the basis at the axes, and its orthonormality under the
    replay's own directions"""
    seq = f32([0.9, 0.9, 0.9, -0.8, 0.7, 0.6, 0.1, -0.2, 0.3] + [0.0] * 15)
    b, tries = ref.unit_sphere_point(lambda done, m: seq[3 * done:3 * (done + m)])
    assert tries == 3 and list(b) == [f32(0.1), f32(-0.2), f32(0.3)]
    np.testing.assert_array_equal(ref.unit_vector(f32([[0, 0, 2.0], [-3.0, 0, 0]])), f32([[0, 0, 1], [-1, 0, 0]]))
    Y = ref.sh9(f32([[1, 0, 0], [0, 1, 0], [0, 0, 1]])).astype(np.float64)
    np.testing.assert_allclose(Y[0], [0.282095, 0, 0, 0.488603, 0, 0, -0.315392, 0, 0.546274], atol=1e-7)
    np.testing.assert_allclose(Y[1], [0.282095, 0.488603, 0, 0, 0, 0, -0.315392, 0, -0.546274], atol=1e-7)
    np.testing.assert_allclose(Y[2], [0.282095, 0, 0.488603, 0, 0, 0, 2 * 0.315392, 0, 0], atol=1e-7)
    dirs, keys = ref.directions(oracle, make_probes(np.zeros((40, 3), f32)), seed=9, first_index=3, samples_per_ray=50, first_sample=2)
    assert dirs.shape == (40, 50, 3) and list(keys["sample"][0][:3]) == [2, 3, 4] and keys["seed"][7, 0] == ref.ray_seed(9, 10)
    np.testing.assert_allclose(np.linalg.norm(dirs.astype(np.float64), axis=-1), 1.0, atol=1e-6)
    assert 1.6 < (keys["ctr"] / 3).mean() < 2.3                      # 6 / pi tries on average
    Y = ref.sh9(dirs.reshape(-1, 3)).astype(np.float64)
    gram = 4 * np.pi * (Y.T @ Y) / len(Y)                            # 2000 uniform directions: the identity within sampling error
    np.testing.assert_allclose(gram, np.eye(9), atol=0.12)


def test_the_skys_closed_form_through_the_emulator(emu_probes, host_scenes):
    """the GPU closed-form test's inputs on the CPU: 4 probes with tmax = 0 (no walk: every sample is the sky along u), 16384 samples,
    every one of the 27 means within 0.05 of its expectation; and vk_probe_eval on the result is the sky's radiance and irradiance / pi"""
    hs, cam = host_scenes("random_spheres_iow")
    probes = make_probes(np.zeros((4, 3), f32), tmax=0.0)
    kw = dict(seed=2024, first_index=7, samples_per_ray=16384, max_depth=50, integrator=ffi.VK_INTEGRATOR_SCATTER,
              background=ffi.VK_BACKGROUND_SKY)
    samples, dirs, _ = emu_probes.probe_samples(hs.desc, probes, **kw)
    assert (np.abs(ref.sh9(dirs[..., :3])[..., None] * samples[..., None, :3]) <= 1.1).all()
    sh, clamped, _ = ref.exact_probes(samples, dirs)
    err = np.abs(sh - ref.sky_expected()[None])
    print(f"\n   max |sh - E[sh]| over 4 x 27 values: {err.max():.4f}")
    assert clamped == 0 and (err <= 0.05).all(), err.max()
    a, b = 1.0 + 0.5 * (ref.SKY_K - 1.0), 0.5 * (ref.SKY_K - 1.0)
    for n in ([0, 1, 0], [0, -1, 0], [1, 0, 0]):
        for mode, slope in ((0, 1.0), (1, 2.0 / 3.0)):     # (1e-5: the basis constants' own rounding, tests/test_probes_abi.py)
            assert (np.abs(probe_eval(sh[0], n, mode) - (a + slope * b * n[1])) <= ref.eval_band(n, mode, 0.05) + 1e-5).all()
