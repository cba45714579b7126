"""Path batches on the device: the compaction alone through vk_debug_compact_paths against tests/paths_ref.py on every output byte; THE
CONTRACT — a batch stepped to its end is the radiance query's sample, radiance and counter, in every scene of the shade tests' set,
ConstantMedium included — stepped one bounce a call and in one call; every bounce's live paths against the host loop (without media)
and the emulator loop (with media); batch sizes around a wave, a handle begun twice, capacity == n and > n; cull; results mid-loop;
refusals; no side effect on vk_render or a vk_progress handle; two handles on one scene."""
import ctypes as C

import numpy as np
import pytest

import paths_ref as P
import shade_ref as S
from vecchio_amd import DeviceScene, ffi
from vecchio_amd.scene import PATH_STATE_DTYPE, RAY_DTYPE, make_path_states

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="session")
def emu_paths(built):
    import emu_paths_ffi
    emu_paths_ffi.load()
    return emu_paths_ffi


def fresh(rays, sample=0):
    return make_path_states(len(rays), S.SEED, S.FIRST, sample)


def assert_live_equal(got, want, what):
    """(ids, rays, states) byte for byte, a NaN's payload aside in the float words"""
    assert np.array_equal(got[0], np.asarray(want[0], np.uint32)), what
    for g, w, dt, words in ((got[1], want[1], RAY_DTYPE, 8), (got[2], want[2], PATH_STATE_DTYPE, 12)):
        g = np.ascontiguousarray(g, dt).view(np.uint32).reshape(-1, words)
        w = np.ascontiguousarray(w, dt).view(np.uint32).reshape(-1, words)
        assert g.shape == w.shape, what
        bad = (g != w) & ~(np.isnan(g.view(f32)) & np.isnan(w.view(f32)))
        if words == 12:
            bad[:, [3, 7, 8, 9, 10, 11]] = (g != w)[:, [3, 7, 8, 9, 10, 11]]      # depth, counter, seed, pixel, sample: integers
        assert not bad.any(), f"{what}: item {int(np.argwhere(bad.any(1))[0, 0])} differs"


# ---------------------------------------------------------------- the compaction alone
@pytest.fixture(scope="module")
def any_scene(device, host_scenes):
    desc, _, _ = S.scene("builder", "cornell_box", host_scenes)
    ds = DeviceScene(desc)
    yield ds
    ds.close()


@pytest.mark.parametrize("n", P.SIZES)
def test_compaction_against_the_reference(n, any_scene):
    for name, status in P.patterns(n).items():
        items, ids, n_ids = P.items_for(status)
        got = any_scene.debug_compact_paths(items, ids, n_ids, canary=P.CANARY)
        P.assert_same(got, P.compact(items, ids, n_ids), f"n {n}, {name}")


def test_compaction_of_nothing_and_a_wild_id(any_scene):
    items, ids, n_ids = P.items_for(P.patterns(4)["all"])
    assert [int(c) for c in any_scene.debug_compact_paths(items[:0], ids[:0], n_ids)[5]] == [0] * 5
    with pytest.raises(RuntimeError, match="an id is not below n_ids"):
        any_scene.debug_compact_paths(items, ids, int(ids.max()))


# ---------------------------------------------------------------- THE CONTRACT, and every bounce
@pytest.mark.parametrize("kind,name", S.ALL_SCENES, ids=[f"{k}-{n}" for k, n in S.ALL_SCENES])
def test_loop_on_scene(kind, name, device, emu_paths, host_scenes):
    desc, cam, p = S.scene(kind, name, host_scenes)
    rays = S.rays_of(cam)
    n = len(rays)
    ds = DeviceScene(desc)
    try:
        with ds.paths(n) as pb:
            for integrator in S.integrators(desc):
                for depth, spp in ((8, 1), (50, 3)):
                    what = f"{kind} {name}, integrator {integrator}, max_depth {depth}"
                    kw = S.shade_kwargs(p, integrator, depth)
                    want = ds.debug_radiance_samples(rays, **S.radiance_kwargs(p, integrator, depth, samples_per_ray=spp))
                    for s in range(spp):
                        # one bounce a call
                        pb.begin(rays, fresh(rays, s), **kw)
                        per_bounce, traced, live = [], 0, n
                        while pb.info().live:
                            st = pb.step(1)
                            assert st.bounces == 1 and st.kernel_launches == 5 and st.kernel_ms > 0 and st.traced == live, what
                            assert st.live + st.missed + st.ended + st.bad == live and st.bad == 0, what
                            traced, live = traced + st.traced, st.live
                            got = pb.read()
                            assert (np.diff(got[0].astype(np.int64)) > 0).all() and len(got[0]) == live, what
                            per_bounce.append(got)
                        assert 1 <= len(per_bounce) <= depth, what
                        S.assert_samples_equal(pb.radiance(), want[:, s], f"{what}, sample {s}, one bounce a call")
                        inf = pb.info()
                        assert inf.started == n and inf.live == 0 and inf.bounces == len(per_bounce) and sum(inf.retired) == n, what
                        assert inf.retired[1] == 0 and inf.retired[3] == 0 and inf.retired[4] == 0, what
                        # one call
                        pb.begin(rays, fresh(rays, s), **kw)
                        st = pb.step(1000)
                        assert st.live == 0 and st.bounces == len(per_bounce) and st.traced == traced and st.kernel_launches == 5 * st.bounces
                        S.assert_samples_equal(pb.radiance(), want[:, s], f"{what}, sample {s}, one call")
                        if depth != 8:
                            continue
                        # every bounce: the host loop without media, the emulator loop with
                        if desc.contents.n_media:
                            _, ref = emu_paths.run(desc, rays, S.SEED, S.FIRST, s, **kw)
                        else:
                            _, bounces = ds.wavefront_radiance(rays, S.SEED, S.FIRST, s, return_bounces=True, **kw)
                            ref = []
                            for b in bounces:
                                go = b["out"]["status"] == ffi.VK_SHADE_SCATTERED
                                ref.append((b["index"][go], b["out"]["next"][go], b["out"]["state"][go]))
                        assert len(ref) == len(per_bounce), what
                        for k, (g, w) in enumerate(zip(per_bounce, ref)):
                            if desc.contents.n_media:
                                assert_live_equal(g, w, f"{what}, bounce {k}")
                            else:      # byte for byte
                                assert np.array_equal(g[0], w[0].astype(np.uint32)), (what, k)
                                assert g[1].tobytes() == np.ascontiguousarray(w[1]).tobytes(), (what, k)
                                assert g[2].tobytes() == np.ascontiguousarray(w[2]).tobytes(), (what, k)
                    assert bits(want[..., 3]).max() > 0, what
    finally:
        ds.close()


# ---------------------------------------------------------------- order and shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_a_second_begin_and_spare_capacity(n, device, host_scenes):
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    rays = np.resize(S.rays_of(cam), n)
    other = np.resize(S.rays_of(cam)[::-1], n)
    kw = S.shade_kwargs(p, p.integrator, 12)
    ds = DeviceScene(desc)
    try:
        want = ds.debug_radiance_samples(rays, **S.radiance_kwargs(p, p.integrator, 12))[:, 0]
        for capacity in (n, n + 77):
            with ds.paths(capacity) as pb:
                assert pb.info().capacity == capacity
                # a first batch, left unfinished: the second is unaffected by it
                pb.begin(other, fresh(other, 1), **kw)
                pb.step(2)
                pb.begin(rays, fresh(rays), **kw)
                assert pb.info().live == n and pb.info().bounces == 0 and sum(pb.info().retired) == 0
                while pb.info().live:
                    pb.step(1)
                    ids = pb.read()[0]
                    assert (np.diff(ids.astype(np.int64)) > 0).all() and (ids < n).all()
                S.assert_samples_equal(pb.radiance(), want, f"n {n}, capacity {capacity}")
                _, status = pb.results()
                assert np.isin(status, (ffi.VK_SHADE_MISS, ffi.VK_SHADE_ENDED)).all()
                # nothing to do: VK_OK
                st = pb.step(3)
                assert st.bounces == 0 and st.traced == 0 and st.kernel_launches == 0
                pb.begin(rays[:0], fresh(rays[:0]), **kw)
                assert pb.info().live == 0 and pb.info().started == 0 and pb.step(1).bounces == 0
                assert len(pb.read()[0]) == 0 and len(pb.results()[1]) == 0
    finally:
        ds.close()


# ---------------------------------------------------------------- cull, results mid-loop
@pytest.mark.parametrize("with_scale", [False, True])
def test_cull_every_second_path_after_bounce_two(with_scale, device, host_scenes):
    """equals the same edit done on the host inside wavefront_loop; the culled ids report VK_PATHS_CULLED with the state they had"""
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    rays = S.rays_of(cam)
    kw = S.shade_kwargs(p, p.integrator, 12)
    ds = DeviceScene(desc)
    try:
        from vecchio_amd.scene import wavefront_loop
        cut = {}

        def shade(r, h, s, calls=[0]):
            out = ds.shade_hits(r, h, s, **kw)
            calls[0] += 1
            if calls[0] == 2:                       # after bounce 2: every second survivor goes, the others' thr is scaled
                go = np.flatnonzero(out["status"] == ffi.VK_SHADE_SCATTERED)
                keep = np.arange(len(go)) % 2 == 0
                scale = np.linspace(0.25, 1.75, len(go)).astype(f32)
                cut.update(keep=keep.astype(np.uint8), scale=scale, states=out["state"][go].copy())
                if with_scale:
                    out["state"]["thr"][go[keep]] = (out["state"]["thr"][go[keep]] * scale[keep, None]).astype(f32)
                out["status"][go[~keep]] = ffi.VK_SHADE_ENDED
            return out

        final, bounces = wavefront_loop(lambda r, s, fi: ds.trace_rays(r, seed=s, first_index=fi), shade, rays, fresh(rays), S.SEED, S.FIRST)
        assert len(bounces) > 3 and len(cut["keep"]) > 8
        with ds.paths(len(rays)) as pb:
            pb.begin(rays, fresh(rays), **kw)
            pb.step(2)
            ids, r0, s0 = pb.read()
            assert s0.tobytes() == cut["states"].tobytes()
            # keep all ones is a no-op on the bytes
            pb.cull(np.ones(len(ids), np.uint8))
            again = pb.read()
            assert again[0].tobytes() == ids.tobytes() and again[1].tobytes() == r0.tobytes() and again[2].tobytes() == s0.tobytes()
            assert pb.info().retired[ffi.VK_PATHS_CULLED] == 0
            pb.cull(cut["keep"], cut["scale"] if with_scale else None)
            gone = ids[cut["keep"] == 0]
            assert pb.info().retired[ffi.VK_PATHS_CULLED] == len(gone) and pb.info().live == len(ids) - len(gone)
            states, status = pb.results()
            assert (status[gone] == ffi.VK_PATHS_CULLED).all() and states[gone].tobytes() == s0[cut["keep"] == 0].tobytes()
            k = 2
            while pb.info().live:
                got = pb.read()
                want = bounces[k]
                assert np.array_equal(got[0], want["index"].astype(np.uint32)), k
                assert got[1].tobytes() == np.ascontiguousarray(want["rays"]).tobytes(), k
                assert got[2].tobytes() == np.ascontiguousarray(want["states"]).tobytes(), k
                pb.step(1)
                k += 1
            assert k == len(bounces)
            states, status = pb.results()
            rest = np.ones(len(rays), bool)
            rest[gone] = False
            assert states[rest].tobytes() == final[rest].tobytes()
            assert (status[gone] == ffi.VK_PATHS_CULLED).all() and np.isin(status[rest], (ffi.VK_SHADE_MISS, ffi.VK_SHADE_ENDED)).all()
    finally:
        ds.close()


def test_results_mid_loop_and_a_null_keep(device, host_scenes):
    desc, cam, p = S.scene("builder", "final_scene", host_scenes)
    rays = S.rays_of(cam)
    ds = DeviceScene(desc)
    try:
        with ds.paths(len(rays) + 3) as pb:
            pb.begin(rays, fresh(rays), **S.shade_kwargs(p, p.integrator, 50))
            states, status = pb.results()                # before the first bounce: everything live, as begun
            assert (status == ffi.VK_PATHS_LIVE).all() and states.tobytes() == fresh(rays).tobytes()
            pb.step(2)
            ids, _, live = pb.read()
            assert 0 < len(ids) < len(rays)
            states, status = pb.results()
            assert (status[ids] == ffi.VK_PATHS_LIVE).all() and states[ids].tobytes() == live.tobytes()
            retired = np.ones(len(rays), bool)
            retired[ids] = False
            assert np.isin(status[retired], (ffi.VK_SHADE_MISS, ffi.VK_SHADE_ENDED)).all()
            inf = pb.info()
            assert inf.retired[0] + inf.retired[2] == retired.sum() and inf.live == len(ids) and inf.bounces == 2
            assert ds._lib.vk_paths_cull(pb._h, None, None) == ffi.VK_ERR_BAD_ARG and b"null keep" in ds._lib.vk_last_error()
            assert ds._lib.vk_paths_step(pb._h, 0, None) == ffi.VK_ERR_BAD_ARG and b"max_bounces" in ds._lib.vk_last_error()
            assert pb.read()[2].tobytes() == live.tobytes()
            pb.step(1000)
            assert ds._lib.vk_paths_cull(pb._h, None, None) == ffi.VK_OK          # nothing live: nothing asked
    finally:
        ds.close()


# ---------------------------------------------------------------- refusals that need a scene
def test_refusals_in_vk_renders_words(device, host_scenes):
    lib = device

    def refused(desc, cam, p, integrator, words):
        ds = DeviceScene(desc)
        try:
            rays = S.rays_of(cam)
            with ds.paths(len(rays)) as pb:
                with pytest.raises(RuntimeError, match="status 2") as e:
                    pb.begin(rays, fresh(rays), **S.shade_kwargs(p, integrator, 8))
                assert words in str(e.value)
                # the handle is as it was: not begun
                ids = np.full(4, 0x77, np.uint32)
                for call in (lambda: lib.vk_paths_step(pb._h, 1, None), lambda: lib.vk_paths_read(pb._h, ids.ctypes.data, None, None),
                             lambda: lib.vk_paths_cull(pb._h, ids.ctypes.data, None)):
                    assert call() == ffi.VK_ERR_BAD_ARG and b"before vk_paths_begin" in lib.vk_last_error()
                assert (ids == 0x77).all() and pb.info().started == 0
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
    # vk_shade_hits' own words for the parameters, n above the capacity, null arrays
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    ds = DeviceScene(desc)
    try:
        rays = S.rays_of(cam)
        states = fresh(rays)
        with ds.paths(16) as pb:
            sp = DeviceScene.shade_params(**S.shade_kwargs(p, p.integrator, 8))
            r, s = rays.ctypes.data, states.ctypes.data
            bad = DeviceScene.shade_params(**S.shade_kwargs(p, p.integrator, 8))
            bad.flags = 1
            worse = DeviceScene.shade_params(**S.shade_kwargs(p, 2, 8))
            for args, word in (((pb._h, None, r, s, 4), b"null argument (scene or shade parameters)"), ((pb._h, C.byref(bad), r, s, 4), b"shade flags must be 0"),
                               ((pb._h, C.byref(worse), r, s, 4), b"bad integrator/background"), ((pb._h, C.byref(sp), None, s, 4), b"null rays"),
                               ((pb._h, C.byref(sp), r, None, 4), b"null rays"), ((pb._h, C.byref(sp), r, s, 17), b"exceeds the path batch's capacity")):
                assert lib.vk_paths_begin(*args) == ffi.VK_ERR_BAD_ARG, word
                assert word in lib.vk_last_error(), lib.vk_last_error()
            assert lib.vk_paths_step(pb._h, 1, None) == ffi.VK_ERR_BAD_ARG            # still not begun
            assert lib.vk_paths_begin(pb._h, C.byref(sp), r, s, 16) == ffi.VK_OK
    finally:
        ds.close()


# ---------------------------------------------------------------- scene state, lifecycle
def test_a_path_batch_leaves_the_render_and_a_progress_handle_alone(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    p = hs.params(96, 4, 20, seed=3)
    kw = S.shade_kwargs(p, p.integrator, 20)
    rays = S.rays_of(cam)
    ds = DeviceScene(hs.desc)
    try:
        def run(pb):
            pb.begin(rays, fresh(rays), **kw)
            pb.step(1000)
            return pb.radiance()

        before, _ = ds.render(cam, p)
        ms, requeued = ds.last_kernel_ms(), ds.last_requeued_samples()
        launches = [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)]
        hits = ds.trace_rays(rays, S.SEED, S.FIRST)
        with ds.paths(len(rays)) as pb:
            first = run(pb)
            assert ds.last_kernel_ms() == ms and ds.last_requeued_samples() == requeued
            assert [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)] == launches and launches
            after, _ = ds.render(cam, p)
            np.testing.assert_array_equal(bits(before), bits(after))
            np.testing.assert_array_equal(bits(run(pb)), bits(first))
            np.testing.assert_array_equal(bits(ds.trace_rays(rays, S.SEED, S.FIRST)), bits(hits))
            # a progress handle interrupted by a path batch is one that was not
            with ds.progress(cam, p) as pr:
                pr.step(2)
                moments = pr.moments()[0].copy()
                info = bytes(pr.info())
                run(pb)
                assert bytes(pr.info()) == info
                np.testing.assert_array_equal(pr.moments()[0], moments)
                interrupted, _ = pr.step(2)
            with ds.progress(cam, p) as pr:
                pr.step(2)
                plain, _ = pr.step(2)
            np.testing.assert_array_equal(bits(interrupted), bits(plain))
    finally:
        ds.close()


def test_two_handles_used_alternately_and_destroy_null(device, host_scenes):
    desc, cam, p = S.scene("builder", "final_scene", host_scenes)
    a_rays = S.rays_of(cam)
    b_rays = a_rays[::-1].copy()
    kw = S.shade_kwargs(p, p.integrator, 50)
    ds = DeviceScene(desc)
    try:
        ds._lib.vk_paths_destroy(None)
        want_a = ds.debug_radiance_samples(a_rays, **S.radiance_kwargs(p, p.integrator, 50))[:, 0]
        want_b = ds.debug_radiance_samples(b_rays, **S.radiance_kwargs(p, p.integrator, 50, samples_per_ray=2))[:, 1]
        with ds.paths(len(a_rays)) as a, ds.paths(len(b_rays) + 5) as b:
            a.begin(a_rays, fresh(a_rays), **kw)
            b.begin(b_rays, fresh(b_rays, 1), **kw)
            while a.info().live or b.info().live:
                a.step(1)
                b.step(2)
            S.assert_samples_equal(a.radiance(), want_a, "handle a")
            S.assert_samples_equal(b.radiance(), want_b, "handle b")
    finally:
        ds.close()
