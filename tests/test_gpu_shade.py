"""Shade queries on the device: the loop of vk_shade_hits' contract (DeviceScene.wavefront_radiance: vk_trace_rays and vk_shade_hits in
turn) against the radiance query's per-sample hook on the scenes and rays of tests/test_shade_emu.py, bit for bit — the record form of
vk_trace.h shade_core (shade_hits_kernel) against the walk form of the same body (radiance_kernel); vk_shade_hits against
the emulator on identical inputs in the scenes with media and for bad hits; batch sizes around a wave, a cut batch, a chunk cut;
refusals; no side effect on vk_render or a vk_progress handle."""
import ctypes as C

import numpy as np
import pytest

import shade_ref as S
from test_shade_emu import bad_hit_batch, check_bad_hits
from vecchio_amd import DeviceScene, ffi
from vecchio_amd.scene import HIT_DTYPE, PATH_STATE_DTYPE, RAY_DTYPE, SHADED_DTYPE, make_path_states

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="session")
def emu_shade(built):
    import emu_shade_ffi
    emu_shade_ffi.load()
    return emu_shade_ffi


# ---------------------------------------------------------------- the contract on the device
@pytest.mark.parametrize("kind,name", S.ALL_SCENES, ids=[f"{k}-{n}" for k, n in S.ALL_SCENES])
def test_loop_on_scene(kind, name, device, emu_shade, host_scenes):
    """without media: the loop is the radiance query's sample (1 sample at max_depth 8, samples 0..2 at max_depth 50), radiance and
    counter.  With media: every bounce's vk_shade_hits is the emulator's on the same rays, hits (vk_trace_rays') and states, all 96 bytes."""
    desc, cam, p = S.scene(kind, name, host_scenes)
    rays = S.rays_of(cam)
    ds = DeviceScene(desc)
    try:
        for integrator in S.integrators(desc):
            for depth, spp in ((8, 1), (50, 3)):
                what = f"{kind} {name}, integrator {integrator}, max_depth {depth}"
                kw = S.shade_kwargs(p, integrator, depth)
                if desc.contents.n_media:
                    got, bounces = ds.wavefront_radiance(rays, S.SEED, S.FIRST, 0, return_bounces=True, **kw)
                    assert 1 <= len(bounces) <= depth
                    for k, b in enumerate(bounces):
                        assert np.isin(b["out"]["status"], S.STATUSES[:3]).all(), what
                        S.assert_shaded_equal(b["out"], emu_shade.shade_hits(desc, b["rays"], b["hits"], b["states"], **kw), f"{what}, bounce {k}")
                        assert b["shade"].samples == len(b["rays"]) and b["shade"].kernel_launches == 1 and b["shade"].kernel_ms > 0
                    continue
                want = ds.debug_radiance_samples(rays, **S.radiance_kwargs(p, integrator, depth, samples_per_ray=spp))
                for s in range(spp):
                    got = ds.wavefront_radiance(rays, S.SEED, S.FIRST, s, **kw)
                    S.assert_samples_equal(got, want[:, s], f"{what}, sample {s}")
                assert bits(want[..., 3]).max() > 0, what
    finally:
        ds.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_around_a_wave(n, device, host_scenes):
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    rays = np.resize(S.rays_of(cam), n)
    ds = DeviceScene(desc)
    try:
        want = ds.debug_radiance_samples(rays, **S.radiance_kwargs(p, p.integrator, 12))
        S.assert_samples_equal(ds.wavefront_radiance(rays, S.SEED, S.FIRST, 0, **S.shade_kwargs(p, p.integrator, 12)), want[:, 0], f"n {n}")
    finally:
        ds.close()


def traced(ds, cam, sample=1):
    """a traced batch with mid-path states: (rays, hits, states)"""
    rays = S.rays_of(cam)
    hits = ds.trace_rays(rays, S.SEED, S.FIRST)
    states = make_path_states(len(rays), S.SEED, S.FIRST, sample)
    states["thr"] = f32([0.5, 0.25, 0.125]); states["acc"] = f32([1.0, 2.0, 3.0]); states["depth"] = 3; states["counter"] = 11
    return rays, hits, states


def test_a_cut_batch_and_a_chunk_cut(device, emu_shade, host_scenes):
    """one batch in two pieces gives the bytes of the uncut batch; so does a batch longer than the staging chunk of 2^19 items (the
    batch repeated: an item's result depends on the item alone)"""
    desc, cam, p = S.scene("builder", "final_scene", host_scenes)
    kw = S.shade_kwargs(p, p.integrator, 50)
    ds = DeviceScene(desc)
    try:
        rays, hits, states = traced(ds, cam)
        whole, st = ds.shade_hits(rays, hits, states, return_stats=True, **kw)
        assert st.samples == len(rays) and st.kernel_launches == 1 and st.kernel_ms > 0
        S.assert_shaded_equal(whole, emu_shade.shade_hits(desc, rays, hits, states, **kw), "against the emulator")
        cut = 77
        parts = [ds.shade_hits(rays[a:b], hits[a:b], states[a:b], **kw) for a, b in ((0, cut), (cut, len(rays)))]
        np.testing.assert_array_equal(bits(np.concatenate(parts)), bits(whole))
        n = (1 << 19) + 65
        big, st = ds.shade_hits(np.resize(rays, n), np.resize(hits, n), np.resize(states, n), return_stats=True, **kw)
        assert st.samples == n and st.kernel_launches == 2
        np.testing.assert_array_equal(bits(big), bits(np.resize(whole, n)))
    finally:
        ds.close()


@pytest.mark.parametrize("kind,name", [("builder", "cornell_box"), ("builder", "final_scene")])
def test_bad_hits_against_the_emulator(kind, name, device, emu_shade, host_scenes):
    """hit = 2 and material = the material count: BAD_HIT, the state copied through, the neighbours untouched — defined behaviour that
    reads no table, the emulator's bytes"""
    desc, cam, p = S.scene(kind, name, host_scenes)
    kw = S.shade_kwargs(p, p.integrator, 50)
    ds = DeviceScene(desc)
    try:
        rays, hits, states, bad, where = bad_hit_batch(desc, cam, lambda r: ds.trace_rays(r, S.SEED, S.FIRST))
        good, spoiled = ds.shade_hits(rays, hits, states, **kw), ds.shade_hits(rays, bad, states, **kw)
        check_bad_hits(good, spoiled, states, where, f"{kind} {name}")
        S.assert_shaded_equal(spoiled, emu_shade.shade_hits(desc, rays, bad, states, **kw), f"{kind} {name} against the emulator")
        bad["material"][where[1]] = 0xFFFFFFFF
        bad["hit"][where[0]] = 0xFFFFFFFF
        spoiled = ds.shade_hits(rays, bad, states, **kw)
        check_bad_hits(good, spoiled, states, where, f"{kind} {name}, extreme")
        S.assert_shaded_equal(spoiled, emu_shade.shade_hits(desc, rays, bad, states, **kw), f"{kind} {name}, extreme, against the emulator")
    finally:
        ds.close()


# ---------------------------------------------------------------- refusals that need a scene
def test_unsupported_in_vk_renders_words(device, host_scenes):
    lib = device

    def refused(desc, cam, p, integrator, words):
        ds = DeviceScene(desc)
        try:
            rays, hits, states = traced(ds, cam)
            out = np.zeros(len(rays), SHADED_DTYPE)
            out.view(np.uint8)[:] = 0x77
            with pytest.raises(RuntimeError, match="status 2") as e:
                ds.shade_hits(rays, hits, states, out=out, **S.shade_kwargs(p, integrator, 8))
            assert words in str(e.value) and (out.view(np.uint8) == 0x77).all()
            img = np.zeros((p.height, p.width, 3), f32)
            q = ffi.RenderParams.from_buffer_copy(p)
            q.integrator = integrator
            assert lib.vk_render(ds._h, C.byref(cam), C.byref(q), img.ctypes.data_as(C.c_void_p), None) == ffi.VK_ERR_UNSUPPORTED
            assert words in lib.vk_last_error().decode()
        finally:
            ds.close()

    desc, cam, p = S.scene("builder", "random_spheres_iow", host_scenes)              # no lights
    refused(desc, cam, p, ffi.VK_INTEGRATOR_PDF, "PDF integrator with an empty lights list")
    desc, cam, p = S.scene("shade", "everything_lit", host_scenes)                    # a SpecDiffuse
    refused(desc, cam, p, ffi.VK_INTEGRATOR_SCATTER, "SpecDiffuse has no Material::scatter")


# ---------------------------------------------------------------- scene state
def test_a_shade_query_leaves_the_render_and_a_progress_handle_alone(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    p = hs.params(96, 4, 20, seed=3)
    kw = S.shade_kwargs(p, p.integrator, 20)
    ds = DeviceScene(hs.desc)
    try:
        rays, hits, states = traced(ds, cam)
        before, _ = ds.render(cam, p)
        ms, requeued = ds.last_kernel_ms(), ds.last_requeued_samples()
        launches = [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)]
        first = ds.shade_hits(rays, hits, states, **kw)
        assert ds.last_kernel_ms() == ms and ds.last_requeued_samples() == requeued
        assert [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)] == launches and launches
        after, _ = ds.render(cam, p)
        np.testing.assert_array_equal(bits(before), bits(after))
        np.testing.assert_array_equal(bits(ds.shade_hits(rays, hits, states, **kw)), bits(first))
        # a progress handle interrupted by a shade call is one that was not
        with ds.progress(cam, p) as pr:
            pr.step(2)
            run = pr.moments()[0].copy()
            info = bytes(pr.info())
            ds.shade_hits(rays, hits, states, **kw)
            assert bytes(pr.info()) == info
            np.testing.assert_array_equal(pr.moments()[0], run)
            interrupted, _ = pr.step(2)
        with ds.progress(cam, p) as pr:
            pr.step(2)
            plain, _ = pr.step(2)
        np.testing.assert_array_equal(bits(interrupted), bits(plain))
    finally:
        ds.close()


def test_no_items(device, host_scenes):
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    ds = DeviceScene(desc)
    try:
        out, st = ds.shade_hits(np.zeros(0, RAY_DTYPE), np.zeros(0, HIT_DTYPE), np.zeros(0, PATH_STATE_DTYPE), return_stats=True,
                                **S.shade_kwargs(p, p.integrator, 8))
        assert out.shape == (0,) and st.samples == 0 and st.kernel_launches == 0
    finally:
        ds.close()
