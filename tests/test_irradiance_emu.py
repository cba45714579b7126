"""Irradiance queries on the CPU: vk_trace.h irradiance_sample (through tests/emu/emu_irradiance.cpp) against the chain of
tests/irradiance_ref.py — the oracle's draws and sine / cosine, a numpy replay of the direction, then the radiance query's per-sample
path (radiance_sample through tests/emu/emu_radiance.cpp, which tests/test_radiance_emu.py holds to the oracle) on the replayed ray with
the stream resumed behind the direction's two draws.  Every comparison is bit for bit (a NaN's payload aside).  193 points x 4 samples
per scene and integrator; tests/test_gpu_irradiance.py runs the chain on the device."""
import numpy as np
import pytest

import irradiance_ref as ref
import special_scenes
from test_emu_parity import BUILDER_SCENES

f32 = np.float32
N, SPP = 193, 4


@pytest.fixture(scope="session")
def emu_irradiance(built):
    import emu_irradiance_ffi
    emu_irradiance_ffi.load()
    return emu_irradiance_ffi


@pytest.fixture(scope="session")
def emu_radiance(built):
    import emu_radiance_ffi
    emu_radiance_ffi.load()
    return emu_radiance_ffi


def through_the_radiance_path(oracle, emu_radiance, desc, pts, kw):
    """(replayed directions, the samples the radiance path gives for them): kw's window of every point"""
    rdirs, keys = ref.directions(oracle, pts, **kw)
    want, _ = emu_radiance.radiance_samples(desc, ref.replayed_rays(pts, rdirs), keys.reshape(-1),
                                            **dict(kw, samples_per_ray=1, first_sample=0, first_index=0))
    return rdirs, want.reshape(len(pts), kw["samples_per_ray"], 4)


def run_chain(oracle, emu_irradiance, emu_radiance, desc, cam, p, what):
    pts = ref.oracle_points(oracle, desc, cam, p, N)
    for integ in ref.integrators_allowed(desc, p.integrator):
        kw = ref.params_kwargs(p, seed=p.seed + 17, first_index=2 ** 40 + 5, samples_per_ray=SPP, max_depth=50, integrator=integ)
        samples, dirs = emu_irradiance.irradiance_samples(desc, pts, **kw)
        # (a) the directions are the replay's; (b) the samples are the radiance path's on the replayed rays and resumed streams
        rdirs, want = through_the_radiance_path(oracle, emu_radiance, desc, pts, kw)
        ref.assert_same_floats(dirs[..., :3], rdirs, f"{what} integrator {integ}: directions")
        assert not ref.bits(dirs[..., 3]).any()
        ref.assert_same_samples(samples, want, f"{what} integrator {integ}: samples")
        assert ref.bits(samples[..., 3]).min() >= 2 and ref.bits(samples[..., 3]).max() > 2 and np.isfinite(dirs).all()
        # (c) the window [3, 8) is rows 3..7 of the window [0, 8)
        full, fdirs = emu_irradiance.irradiance_samples(desc, pts, **dict(kw, samples_per_ray=8))
        win, wdirs = emu_irradiance.irradiance_samples(desc, pts, **dict(kw, samples_per_ray=5, first_sample=3))
        ref.assert_same_samples(win, full[:, 3:8], f"{what} integrator {integ}: window")
        ref.assert_same_floats(wdirs, fdirs[:, 3:8], f"{what} integrator {integ}: window directions")
        ref.assert_same_samples(full[:, :SPP], samples, f"{what} integrator {integ}: the first rows of a longer window")
        # (d) max_depth 0: (0,0,0) without a draw
        zero, zdirs = emu_irradiance.irradiance_samples(desc, pts, **dict(kw, max_depth=0))
        assert not ref.bits(zero).any() and not ref.bits(zdirs).any()
        # (e) a finite tmax on every third point — at or below VK_RAY_TMIN (no walk), below the nearest surface of most points, and
        # far enough to reach one — is the radiance path's tmax
        cut = pts.copy()
        cut["tmax"][::3] = np.resize(f32([0.001, 0.004, 0.3, 25.0, np.nan]), len(cut["tmax"][::3]))
        csamples, cdirs = emu_irradiance.irradiance_samples(desc, cut, **kw)
        _, cwant = through_the_radiance_path(oracle, emu_radiance, desc, cut, kw)
        ref.assert_same_floats(cdirs[..., :3], rdirs, f"{what} integrator {integ}: directions with a tmax")
        ref.assert_same_samples(csamples, cwant, f"{what} integrator {integ}: samples with a tmax")
        rest = np.ones(len(pts), bool)
        rest[::3] = False
        ref.assert_same_samples(csamples[rest], samples[rest], f"{what} integrator {integ}: points whose tmax stayed infinite")
        # a ray that is not walked sees the background at once: its stream stands where the direction's draws left it
        assert (ref.bits(csamples[0:len(pts):15, :, 3]) == 2).all()


@pytest.mark.parametrize("name", BUILDER_SCENES)
def test_builder_scene(name, oracle, emu_irradiance, emu_radiance, host_scenes):
    hs, cam = host_scenes(name)
    run_chain(oracle, emu_irradiance, emu_radiance, hs.desc, cam, hs.params(20, 1, 50, height=12), name)


@pytest.mark.parametrize("name", sorted(special_scenes.ALL))
def test_special_scene(name, oracle, emu_irradiance, emu_radiance, built):
    d, desc, cam, p = special_scenes.ALL[name]()
    run_chain(oracle, emu_irradiance, emu_radiance, desc, cam, p, name)


def test_the_replay_against_closed_forms(oracle):
    """the numpy restatement itself: the frame of a normal along +z and along +x, unit length and orthogonality, the cosine-weighted
    direction's own length and hemisphere"""
    u, v, w = ref.onb_from_w(f32([[0, 0, 2.0], [-3.0, 0, 0]]))
    np.testing.assert_array_equal(w, f32([[0, 0, 1], [-1, 0, 0]]))
    np.testing.assert_array_equal(v, f32([[0, 1, 0], [0, 0, -1]]))          # w x (1,0,0) and w x (0,1,0)
    np.testing.assert_array_equal(u, f32([[-1, 0, 0], [0, -1, 0]]))
    rng = np.random.default_rng(2)
    nrm = (rng.normal(size=(50, 3)) * rng.uniform(0.1, 30, (50, 1))).astype(f32)
    pts = ref.make_rays(np.zeros((50, 3), f32), nrm)
    dirs, keys = ref.directions(oracle, pts, seed=9, first_index=3, samples_per_ray=6, first_sample=2)
    assert dirs.shape == (50, 6, 3) and (keys["ctr"] == 2).all() and list(keys["sample"][0]) == [2, 3, 4, 5, 6, 7]
    assert keys["seed"][7, 0] == ref.ray_seed(9, 10)
    np.testing.assert_allclose(np.linalg.norm(dirs.astype(np.float64), axis=-1), 1.0, atol=1e-5)
    unit = nrm.astype(np.float64) / np.linalg.norm(nrm.astype(np.float64), axis=1, keepdims=True)
    cos = (dirs.astype(np.float64) * unit[:, None, :]).sum(-1)
    assert (cos > -1e-6).all() and 0.55 < cos.mean() < 0.78               # E[cos] = 2/3 under the density cos / pi
