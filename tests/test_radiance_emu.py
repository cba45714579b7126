"""Radiance queries on the CPU: vk_trace.h radiance_sample (through tests/emu/emu_radiance.cpp, on the tree view the library promises, the
kernel instance chosen as the launcher chooses it) against the oracle through the bridge of tests/radiance_ref.py — every sample of a
20 x 12 x 4 frame: the oracle's primary ray with the stream resumed behind the camera's draws must give the oracle's sample.
tests/test_gpu_radiance.py runs the bridge on the device."""
import numpy as np
import pytest

import radiance_ref
import special_scenes
from test_emu_parity import BUILDER_SCENES
from vecchio_amd.scene import make_rays

W, H, SPP = 20, 12, 4


@pytest.fixture(scope="session")
def emu_radiance(built):
    import emu_radiance_ffi
    emu_radiance_ffi.load()
    return emu_radiance_ffi


def run_bridge(oracle, emu_radiance, desc, cam, p):
    rays, keys, ref = radiance_ref.bridge(oracle, desc, cam, p)
    got, _ = emu_radiance.radiance_samples(desc, rays, keys, **radiance_ref.radiance_kwargs(p))
    return radiance_ref.compare(ref, got)


@pytest.mark.parametrize("name", BUILDER_SCENES)
def test_builder_scene(name, oracle, emu_radiance, host_scenes):
    hs, cam = host_scenes(name)
    run_bridge(oracle, emu_radiance, hs.desc, cam, hs.params(W, SPP, 50, height=H))


@pytest.mark.parametrize("name", sorted(special_scenes.ALL))
def test_special_scene(name, oracle, emu_radiance, built):
    d, desc, cam, p = special_scenes.ALL[name]()
    p.width, p.height, p.samples_per_pixel, p.max_depth = W, H, SPP, 50
    run_bridge(oracle, emu_radiance, desc, cam, p)


@pytest.mark.parametrize("depth", [1, 3])
def test_cornell_box_depth_limit(depth, oracle, emu_radiance, host_scenes):
    hs, cam = host_scenes("cornell_box")
    run_bridge(oracle, emu_radiance, hs.desc, cam, hs.params(W, SPP, depth, height=H, seed=11))


def test_public_stream_rule_and_windows(emu_radiance, host_scenes):
    """keys NULL: sample s of ray i draws from rng_for_sample(seed + GOLDEN * (first_index + i), 0, s) — the same thing as the key
    (that seed, 0, s, 0); the window [3, 8) is rows 3..7 of [0, 8); max_depth 0 is (0,0,0) without a draw"""
    from rays_ref import ray_seed
    from vecchio_amd.scene import KEY_DTYPE
    hs, cam = host_scenes("final_scene")
    o = np.float32(list(cam.origin))
    look = np.float32(list(cam.lower_left_corner)) + np.float32(0.5) * np.float32(list(cam.horizontal)) + \
        np.float32(0.5) * np.float32(list(cam.vertical)) - o
    rng = np.random.default_rng(3)
    rays = make_rays(np.tile(o, (9, 1)), look + rng.normal(scale=40.0, size=(9, 3)).astype(np.float32), 0.5)
    kw = dict(seed=77, first_index=2 ** 40, max_depth=20, integrator=hs.integrator, background=hs.background,
              background_color=hs.background_color)
    full, _ = emu_radiance.radiance_samples(hs.desc, rays, samples_per_ray=8, **kw)
    assert full[..., 3].view(np.uint32).max() > 0
    win, _ = emu_radiance.radiance_samples(hs.desc, rays, samples_per_ray=5, first_sample=3, **kw)
    np.testing.assert_array_equal(win.view(np.uint32), full[:, 3:8].view(np.uint32))
    keys = np.zeros(9, KEY_DTYPE)
    keys["seed"] = [ray_seed(77, 2 ** 40 + i) for i in range(9)]
    keyed, _ = emu_radiance.radiance_samples(hs.desc, rays, keys, samples_per_ray=8, **kw)
    np.testing.assert_array_equal(keyed.view(np.uint32), full.view(np.uint32))
    kw["max_depth"] = 0
    zero, _ = emu_radiance.radiance_samples(hs.desc, rays, samples_per_ray=2, **kw)
    assert not zero.view(np.uint32).any()
