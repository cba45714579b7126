"""Regeneration on the device (vk_regen_*).  THE CONTRACT on every scene of the shade tests' set and each integrator vk_render allows
there: a frame sent through regenerating batches of awkward capacities is vk_render's frame bit for bit, with the exact sums and the
window route's counters.  Per bounce: vk_paths_read after every bounce of a regenerating batch is tests/regen_ref.py's schedule of the
lifetimes, rays and states the window route (vk_film_emit, vk_paths_step one bounce a call) shows on the same frame, byte for byte.  Any
slicing by max_bounces; a capacity at and above the window's size; a capacity that takes the scan two passes; a cull rule between steps;
windows mixed between the two routes and between two regenerating batches; refusals that leave film and batch as they were; no side
effect on vk_render, the launch log, the ray queries or a vk_progress handle; a multi-device scene."""
import ctypes as C

import numpy as np
import pytest

import exact_sums as E
import film_ref as F
import regen_ref as G
import shade_ref as S
import test_gpu_film as GF
from descs import camera
from vecchio_amd import DeviceScene, ffi
from vecchio_amd.scene import PATH_STATE_DTYPE, RAY_DTYPE

pytestmark = pytest.mark.gpu
SPP = 3
CAPACITIES = (63, 64, 65, 255, 256, 257, 773)
bits, frame_params = GF.bits, GF.frame_params
ALL = 0xFFFFFFFF


def finished(info):
    return info.live == 0 and info.remaining == 0


def run(film, pb, win, max_bounces=ALL):
    """a regenerating run of the window to its end: the calls' infos"""
    film.regen_begin(pb, *win)
    infos = [film.regen_step(pb, max_bounces)]
    while not finished(infos[-1]):
        infos.append(film.regen_step(pb, max_bounces))
    return infos


def counters(film):
    i = film.info()
    return (i.emitted, i.deposited, i.dropped, i.clamped, i.skipped)


# ---------------------------------------------------------------- 1. THE CONTRACT
@pytest.mark.parametrize("kind,name", S.ALL_SCENES, ids=[f"{k}-{n}" for k, n in S.ALL_SCENES])
def test_contract_on_scene(kind, name, device, host_scenes):
    desc, cam, p = S.scene(kind, name, host_scenes)
    W, H = p.width, p.height
    n = W * H * SPP
    ds = DeviceScene(desc)
    batches = []
    try:
        batches = [ds.paths(c) for c in CAPACITIES]
        with ds.paths(n) as big:
            for integrator in S.integrators(desc):
                for depth in S.DEPTHS:
                    q = frame_params(p, integrator, SPP, depth)
                    _, dump = GF.render_dump(ds, cam, q)
                    frame, stats = ds.render(cam, q)
                    want_sums, want_clamped = E.frame_sums(dump, W, H, SPP)
                    with ds.film(cam, q) as film:
                        GF.whole_frame(film, big, q)                          # the window route
                        route = counters(film)
                        assert route[3] == stats.clamped_samples == want_clamped
                        for cap, pb in zip(CAPACITIES, batches):
                            what = f"{kind} {name}, integrator {integrator}, max_depth {depth}, capacity {cap}"
                            film.reset()
                            img = film.render_regen(pb)
                            assert np.array_equal(bits(img), bits(frame)), what
                            assert np.array_equal(film.debug_sums(), want_sums), what
                            inf = film.info()
                            assert counters(film) == route and inf.deposits == 0, what
                            assert inf.emitted == n == inf.deposited + inf.dropped + inf.skipped, what
                            pi = pb.info()
                            assert pi.started == n and pi.live == 0 and sum(pi.retired) == n and pi.retired[1] == 0, what
    finally:
        for b in batches:
            b.close()
        ds.close()


def test_capacity_one(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    q = hs.params(5, SPP, 8, seed=3, height=4)
    ds = DeviceScene(hs.desc)
    try:
        frame, stats = ds.render(cam, q)
        with ds.film(cam, q) as film, ds.paths(1) as pb:
            film.regen_begin(pb, 0, 0, 5, 4, 0, SPP)
            traced = bounces = 0
            while True:
                info = film.regen_step(pb, 7)
                traced, bounces = traced + info.traced, bounces + info.bounces
                assert info.live <= 1 and info.kernel_launches <= 6 * info.bounces
                if finished(info):
                    break
            assert traced == bounces >= 5 * 4 * SPP and pb.info().bounces == bounces            # one path a bounce
            assert np.array_equal(bits(film.resolve()), bits(frame)) and film.info().clamped == stats.clamped_samples
            assert film.regen_step(pb, 1).bounces == 0                                           # a step on a finished run does nothing
            assert film.info().emitted == 5 * 4 * SPP
    finally:
        ds.close()


# ---------------------------------------------------------------- 2. per bounce
def lens_camera():
    return camera((478, 278, -600), (278, 278, 0), vfov=40.0, aspect=24 / 16, aperture=8.0, focus=600.0, t0=0.25, t1=1.0)


def window_route_history(film, big, win):
    """the window emitted whole and stepped one bounce a call: (ids, rays, states) live after 0, 1, 2, ... bounces"""
    film.emit(big, *win)
    hist = [big.read()]
    while big.info().live:
        big.step(1)
        hist.append(big.read())
    film.deposit(big)
    return hist


@pytest.mark.parametrize("which", ["no_media", "constant_medium", "lens_and_shutter"])
def test_every_bounce_is_the_schedule(which, device, host_scenes):
    if which == "no_media":
        desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
        assert desc.contents.n_media == 0
    elif which == "constant_medium":
        desc, cam, p = S.scene("hand", "glass_and_media", host_scenes)
        assert desc.contents.n_media > 0
    else:
        hs, _ = host_scenes("final_scene")
        desc, cam, p = hs.desc, lens_camera(), hs.params(24, SPP, 12, seed=11, height=16)
        assert cam.lens_radius > 0 and cam.time0 < cam.time1 and desc.contents.n_moving_spheres > 0
    q = frame_params(p, spp=SPP, max_depth=12)
    W, H = q.width, q.height
    win = (1, 2, W - 3, H - 3, 0, SPP)
    total = win[2] * win[3] * SPP
    ds = DeviceScene(desc)
    try:
        with ds.film(cam, q) as ref, ds.film(cam, q) as film, ds.paths(total) as big:
            hist = window_route_history(ref, big, win)
            ids_at = [h[0] for h in hist]
            life = G.lifetimes_of(ids_at, total)
            rays_at = np.stack(G.by_id(ids_at, [h[1] for h in hist], total))            # [age][id]
            states_at = np.stack(G.by_id(ids_at, [h[2] for h in hist], total))
            assert life.max() > 2 and len(hist[0][0]) == total
            want_sums, want_counters = ref.debug_sums().tobytes(), counters(ref)
            for cap in (64, 65, 257):
                sched = G.schedule(life, cap)
                film.reset()
                with ds.paths(cap) as pb:
                    film.regen_begin(pb, *win)
                    assert pb.info().live == 0 and pb.info().started == 0 and len(pb.read()[0]) == 0
                    for k, b in enumerate(sched):
                        what = f"{which}, capacity {cap}, bounce {k}"
                        info = film.regen_step(pb, 1)
                        assert info.bounces == 1 and info.traced == len(b["before"]) and info.live == len(b["after"]), what
                        assert info.emitted == int((b["before_age"] == 0).sum()) and info.kernel_launches == (6 if info.emitted else 5), what
                        ids, rays, states = pb.read()
                        assert np.array_equal(ids, b["after"]), what
                        want_r, want_s = rays_at[b["after_age"], b["after"]], states_at[b["after_age"], b["after"]]
                        assert rays.tobytes() == want_r.tobytes() and states.tobytes() == want_s.tobytes(), what
                        assert finished(info) == (k == len(sched) - 1), what
                    assert pb.info().bounces == len(sched) and pb.info().started == total
                    ms = film.regen_last_ms(pb)
                    assert len(ms) == 4 and min(ms) >= 0 and ms[1] > 0 and ms[2] > 0 and ms[3] > 0
                    assert film.debug_sums().tobytes() == want_sums and counters(film) == want_counters, (which, cap)
    finally:
        ds.close()


# ---------------------------------------------------------------- 3. slicing, and a capacity that holds the window
def test_any_slicing_and_a_capacity_at_or_above_the_window(device, host_scenes):
    desc, cam, p = S.scene("builder", "final_scene", host_scenes)
    q = frame_params(p, spp=SPP, max_depth=50)
    W, H = q.width, q.height
    win = (0, 0, W, H, 0, SPP)
    total = W * H * SPP
    ds = DeviceScene(desc)
    try:
        with ds.film(cam, q) as ref, ds.film(cam, q) as film, ds.paths(total) as big, ds.paths(100) as pb, ds.paths(total + 7) as roomy:
            hist = window_route_history(ref, big, win)
            want, route = ref.debug_sums().tobytes(), counters(ref)
            seen = []
            for max_bounces in (1, 3, 1000):
                film.reset()
                infos = run(film, pb, win, max_bounces)
                assert all(i.bounces == max_bounces for i in infos[:-1]) and 1 <= infos[-1].bounces <= max_bounces
                assert film.debug_sums().tobytes() == want and counters(film) == route, max_bounces
                seen.append((bytes(pb.info()), sum(i.traced for i in infos), sum(i.kernel_launches for i in infos)))
            assert seen[0] == seen[1] == seen[2] and len(run(film, pb, (0, 0, 2, 2, 0, 1), 1000)) == 1
            # capacity >= total: the window route's own bounces
            for b in (big, roomy):
                film.reset()
                film.regen_begin(b, *win)
                for k in range(1, len(hist)):
                    info = film.regen_step(b, 1)
                    assert info.emitted == (total if k == 1 else 0) and info.traced == len(hist[k - 1][0])
                    got = b.read()
                    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, hist[k])), k
                assert finished(info) and film.regen_step(b, 5).bounces == 0
                assert film.debug_sums().tobytes() == want and counters(film) == route
    finally:
        ds.close()


def test_a_capacity_that_takes_the_scan_two_passes(device, host_scenes):
    hs, cam = host_scenes("random_spheres_iow")
    q = hs.params(128, 8, 8, seed=4, height=128)
    ds = DeviceScene(hs.desc)
    try:
        frame, stats = ds.render(cam, q)
        with ds.film(cam, q) as film, ds.paths(66000) as pb:
            assert -(-66000 // 256) > 256
            assert np.array_equal(bits(film.render_regen(pb)), bits(frame))
            inf = film.info()
            assert inf.emitted == 128 * 128 * 8 == inf.deposited + inf.dropped and inf.clamped == stats.clamped_samples
    finally:
        ds.close()


# ---------------------------------------------------------------- 4. a cull rule between steps
def rule(ids, states):
    """keep and scale of the live paths, from (id, state.depth) alone"""
    key = (ids.astype(np.uint64) * np.uint64(2654435761) + states["depth"].astype(np.uint64) * np.uint64(40503)) >> np.uint64(5)
    keep = (key % np.uint64(4) != 0).astype(np.uint8)
    return keep, np.full(len(ids), 4.0 / 3.0, np.float32)


def test_a_cull_rule_between_steps(device, host_scenes):
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    q = frame_params(p, spp=SPP, max_depth=20)
    W, H = q.width, q.height
    win = (0, 0, W, H, 0, SPP)
    ds = DeviceScene(desc)
    try:
        with ds.film(cam, q) as ref, ds.film(cam, q) as film, ds.paths(W * H * SPP) as big:
            ref.emit(big, *win)
            while big.step(1).live:
                ids, _, states = big.read()
                big.cull(*rule(ids, states))
            ref.deposit(big)
            culled = big.info().retired[ffi.VK_PATHS_CULLED]
            assert culled > 64 and counters(ref)[1] + counters(ref)[2] == W * H * SPP
            plain, _ = ds.render(cam, q)
            assert not np.array_equal(bits(ref.resolve()), bits(plain))
            for cap in (65, 257):
                with ds.paths(cap) as pb:
                    film.reset()
                    film.regen_begin(pb, *win)
                    while True:
                        info = film.regen_step(pb, 1)
                        if finished(info):
                            break
                        if info.live:
                            ids, _, states = pb.read()
                            film.regen_cull(pb, *rule(ids, states))
                    assert film.debug_sums().tobytes() == ref.debug_sums().tobytes(), cap
                    assert counters(film) == counters(ref) and pb.info().retired[ffi.VK_PATHS_CULLED] == culled, cap
                    assert list(pb.info().retired)[:4] == list(big.info().retired)[:4]
            # render_regen calls a rule between bounces; one that keeps every path leaves vk_render's frame
            calls = []

            def keep_all(b):
                calls.append(int(b.info().live))
                film.regen_cull(b, np.ones(calls[-1], np.uint8))

            film.reset()
            with ds.paths(100) as pb:
                assert np.array_equal(bits(film.render_regen(pb, cull=keep_all)), bits(plain))
            assert len(calls) > 10 and min(calls) >= 1 and max(calls) <= 100
    finally:
        ds.close()


# ---------------------------------------------------------------- 5. mixing
def test_windows_mixed_between_the_routes_and_between_two_regenerating_batches(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    FW, FH = GF.FW, GF.FH
    q = hs.params(FW, SPP, 20, seed=5, height=FH)
    ds = DeviceScene(hs.desc)
    try:
        frame, stats = ds.render(cam, q)
        with ds.film(cam, q) as one, ds.film(cam, q) as many, ds.paths(FW * FH * SPP) as big, ds.paths(70) as a, ds.paths(300) as b:
            GF.whole_frame(one, big, q)
            want = one.debug_sums().tobytes()
            assert np.array_equal(bits(one.resolve()), bits(frame))
            order = np.random.default_rng(12).permutation(len(GF.WINDOWS))
            for k, j in enumerate(order):
                w = GF.WINDOWS[j]
                if k % 2 == 0:
                    run(many, (a, b)[(k // 2) % 2], w, 1 + k)
                else:
                    many.emit(b, *w)
                    assert b.step(100000).live == 0
                    many.deposit(b)
            assert many.debug_sums().tobytes() == want and counters(many) == counters(one)
            assert many.info().deposits == len(GF.WINDOWS) // 2
            # two batches regenerating alternately into one film, for disjoint windows
            many.reset()
            left, right = (0, 0, 17, FH, 0, SPP), (17, 0, FW - 17, FH, 0, SPP)
            many.regen_begin(a, *left)
            many.regen_begin(b, *right)
            done = [False, False]
            while not all(done):
                for i, (pb, nb) in enumerate(((a, 2), (b, 1))):
                    if not done[i]:
                        done[i] = finished(many.regen_step(pb, nb))
            assert many.debug_sums().tobytes() == want and counters(many) == counters(one)
            assert np.array_equal(bits(many.resolve()), bits(frame)) and many.info().clamped == stats.clamped_samples
    finally:
        ds.close()


# ---------------------------------------------------------------- 6. state and refusals
def test_refusals_leave_film_and_batch_as_they_were(device, host_scenes):
    lib = device
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    q = frame_params(p, max_depth=8)
    W, H = q.width, q.height
    ds, other = DeviceScene(desc), DeviceScene(desc)
    try:
        with ds.film(cam, q) as film, ds.film(cam, q) as film2, ds.paths(50) as pb, other.paths(50) as foreign, ds.paths(W * H * SPP) as plain:
            film.regen_begin(pb, 0, 0, W, H, 0, SPP)
            film.regen_step(pb, 2)
            film.emit(plain, 0, 0, W, H, 0, 1)
            plain.step(1)
            assert pb.info().live > 0 and plain.info().live > 0 and film.debug_sums().any()
            keep = np.zeros(W * H, np.uint8)
            info = ffi.RegenInfo()
            info.traced = 99

            def refused(call, word):
                before, sums0 = [bytes(x.info()) for x in (pb, plain, film, film2)], film.debug_sums().tobytes()
                assert call() == ffi.VK_ERR_BAD_ARG, word
                assert word in lib.vk_last_error(), lib.vk_last_error()
                assert [bytes(x.info()) for x in (pb, plain, film, film2)] == before and film.debug_sums().tobytes() == sums0, word
                assert info.traced == 99

            begin = lambda f, b, *w: lib.vk_regen_begin(f, b, C.byref(ffi.FilmWindow(*w)))
            step = lambda f, b, nb=1: lib.vk_regen_step(f, b, nb, C.byref(info))
            cull = lambda f, b: lib.vk_regen_cull(f, b, keep.ctypes.data, None)
            # vk_regen_begin: vk_film_emit's words, but no capacity rule
            refused(lambda: begin(None, pb._h, 0, 0, 2, 2, 0, 1), b"null argument")
            refused(lambda: begin(film._h, None, 0, 0, 2, 2, 0, 1), b"null argument")
            refused(lambda: lib.vk_regen_begin(film._h, pb._h, None), b"null argument")
            refused(lambda: begin(film._h, foreign._h, 0, 0, 2, 2, 0, 1), b"belongs to another scene")
            refused(lambda: begin(film._h, pb._h, W - 3, 0, 4, 2, 0, 1), b"outside the film's frame")
            refused(lambda: begin(film._h, pb._h, 0, 0xFFFFFFFF, 2, 2, 0, 1), b"outside the film's frame")
            refused(lambda: begin(film._h, pb._h, 0, 0, 0, 2, 0, 1), b"empty window")
            refused(lambda: begin(film._h, pb._h, 0, 0, 2, 2, 0, 0), b"empty window")
            refused(lambda: begin(film._h, pb._h, 0, 0, 2, 2, SPP - 1, 2), b"exceeds the film's samples_per_pixel")
            # vk_regen_step and vk_regen_cull
            refused(lambda: step(None, pb._h), b"null argument")
            refused(lambda: step(film._h, None), b"null argument")
            refused(lambda: step(film._h, pb._h, 0), b"max_bounces must be >= 1")
            refused(lambda: step(film._h, foreign._h), b"belongs to another scene")
            refused(lambda: step(film._h, plain._h), b"not regenerating")
            refused(lambda: step(film2._h, pb._h), b"begun with another film")
            refused(lambda: cull(None, pb._h), b"null argument")
            refused(lambda: cull(film._h, None), b"null argument")
            refused(lambda: cull(film._h, foreign._h), b"belongs to another scene")
            refused(lambda: cull(film._h, plain._h), b"not regenerating")
            refused(lambda: cull(film2._h, pb._h), b"begun with another film")
            refused(lambda: lib.vk_regen_cull(film._h, pb._h, None, None), b"null keep with live paths")
            # the existing functions on a regenerating batch
            st, status = np.zeros(W * H * SPP, PATH_STATE_DTYPE), np.zeros(W * H * SPP, np.uint32)
            refused(lambda: lib.vk_paths_step(pb._h, 1, None), b"regenerating")
            refused(lambda: lib.vk_paths_cull(pb._h, keep.ctypes.data, None), b"regenerating")
            refused(lambda: lib.vk_paths_results(pb._h, st.ctypes.data, status.ctypes.data), b"regenerating")
            refused(lambda: lib.vk_film_deposit(film._h, pb._h), b"regenerating")
            assert not st.view(np.uint8).any() and not status.any()
            ms = (C.c_double * 4)(7, 7, 7, 7)
            refused(lambda: lib.vk_debug_regen_last_ms(plain._h, C.byref(ms)), b"no bounce has run since vk_regen_begin")
            assert list(ms) == [7, 7, 7, 7]
            # vk_paths_read and vk_paths_get_info work, and both batches finish as batches that were never bothered
            ids, rays, states = pb.read()
            inf = pb.info()
            assert len(ids) == inf.live and inf.started > ids.max() and len(rays) == len(states) == len(ids) and (np.diff(ids.astype(np.int64)) > 0).all()
            assert inf.bounces == 2 and inf.started - inf.live == sum(inf.retired)
            while not finished(film.regen_step(pb, 3)):
                pass
            refused(lambda: lib.vk_film_deposit(film._h, pb._h), b"regenerating")
            assert plain.step(100000).live == 0
            film.deposit(plain)
            with ds.film(cam, q) as ref:
                GF.whole_frame(ref, plain, frame_params(q, spp=1))
                ref.emit(plain, 0, 0, W, H, 0, SPP)
                assert plain.step(100000).live == 0
                ref.deposit(plain)
                assert ref.debug_sums().tobytes() == film.debug_sums().tobytes() and counters(ref) == counters(film)
            # vk_paths_begin ends a run: the batch then is a plain batch
            film.regen_begin(pb, 0, 0, W, H, 0, 1)
            film.regen_step(pb, 1)
            assert pb.info().live > 0
            some = st[:40].copy()
            some["pixel"], some["acc"] = np.arange(40), 0.25
            pb.begin(np.zeros(40, RAY_DTYPE), some, **S.shade_kwargs(q, q.integrator, 8))
            assert pb.info().started == 40 and pb.info().live == 40
            refused(lambda: step(film._h, pb._h), b"not regenerating")
            pb.cull(np.zeros(40, np.uint8))
            back, status = pb.results()
            assert back.tobytes() == some.tobytes() and (status == ffi.VK_PATHS_CULLED).all()
            film.reset()
            film.deposit(pb)
            assert film.info().deposited == 40 and film.info().deposits == 1
            # and so does vk_film_emit
            film.regen_begin(pb, 0, 0, W, H, 0, 1)
            film.regen_step(pb, 1)
            film.reset()
            film.emit(pb, 0, 0, 5, 5, 0, 2)
            assert pb.step(100000).live == 0
            film.deposit(pb)
            assert film.info().deposited + film.info().dropped == 50
    finally:
        other.close()
        ds.close()


def test_regeneration_leaves_the_render_the_queries_and_a_progress_handle_alone(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    p = hs.params(96, 4, 20, seed=3)
    fq = hs.params(24, SPP, 20, seed=4, height=16)
    rays = S.rays_of(cam)
    ds = DeviceScene(hs.desc)
    multi = None
    try:
        before, _ = ds.render(cam, p)
        ms, requeued = ds.last_kernel_ms(), ds.last_requeued_samples()
        launches = [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)]
        hits = ds.trace_rays(rays, S.SEED, S.FIRST)
        with ds.film(cam, fq) as film, ds.paths(100) as pb:
            film.render_regen(pb)
            first = film.debug_sums().copy()
            assert abs(ds.last_kernel_ms() - ms) < 1e-4 and ds.last_requeued_samples() == requeued
            assert [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)] == launches and launches
            after, _ = ds.render(cam, p)
            np.testing.assert_array_equal(bits(before), bits(after))
            np.testing.assert_array_equal(bits(ds.trace_rays(rays, S.SEED, S.FIRST)), bits(hits))
            with ds.progress(cam, p) as pr:
                pr.step(2)
                moments = pr.moments()[0].copy()
                info = bytes(pr.info())
                film.reset()
                film.render_regen(pb)
                np.testing.assert_array_equal(film.debug_sums(), first)
                assert bytes(pr.info()) == info
                np.testing.assert_array_equal(pr.moments()[0], moments)
                interrupted, _ = pr.step(2)
            with ds.progress(cam, p) as pr:
                pr.step(2)
                plain, _ = pr.step(2)
            np.testing.assert_array_equal(bits(interrupted), bits(plain))
            frame, _ = ds.render(cam, fq)
            assert np.array_equal(bits(film.resolve()), bits(frame))
        # the same frame on a multi-device scene (devices[0] does the work)
        multi = DeviceScene(hs.desc, devices=[0, 0])
        with multi.film(cam, fq) as film, multi.paths(200) as pb:
            assert np.array_equal(bits(film.render_regen(pb)), bits(frame))
            assert film.info().deposits == 0 and film.info().emitted == 24 * 16 * SPP
    finally:
        if multi is not None:
            multi.close()
        ds.close()
