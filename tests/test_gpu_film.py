"""Films on the device.  THE CONTRACT on every scene of the shade tests' set and each integrator vk_render allows there: camera paths
emitted into a path batch and stepped to the end are vk_render's samples, radiance and counter bit for bit, and the deposited, resolved
frame is vk_render's frame bit for bit with its counters.  A frame assembled from shuffled windows of every awkward size through two
batches equals the one-emit frame byte for byte, also on a multi-device scene.  The deposit alone, in both forms, on hand-made states
against tests/film_ref.py.  A roulette between bounces.  Refusals that leave film and batch as they were.  No side effect on vk_render,
the launch log, the ray queries or a vk_progress handle; two films on one scene; reset with a camera."""
import ctypes as C

import numpy as np
import pytest

import exact_sums as E
import film_ref as F
import shade_ref as S
from vecchio_amd import DeviceScene, ffi
from vecchio_amd.scene import RAY_DTYPE

pytestmark = pytest.mark.gpu
f32 = np.float32
SPP = 3
FORMS = (ffi.VK_DEBUG_FILM_DEPOSIT_PLAIN, ffi.VK_DEBUG_FILM_DEPOSIT_RUNS)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frame_params(p, integrator=None, spp=SPP, max_depth=None):
    q = ffi.RenderParams.from_buffer_copy(p)
    q.samples_per_pixel = spp
    if integrator is not None:
        q.integrator = integrator
    if max_depth is not None:
        q.max_depth = max_depth
    return q


def render_dump(ds, cam, q):
    """(vk_debug_render_samples' frame, its dump [pixel * spp + s] = (r, g, b, counter bits))"""
    lib = ds._lib
    lib.vk_debug_render_samples.restype = C.c_int
    lib.vk_debug_render_samples.argtypes = [C.c_void_p, C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_void_p, C.c_void_p]
    img = np.zeros((q.height, q.width, 3), f32)
    dump = np.zeros((q.width * q.height * q.samples_per_pixel, 4), f32)
    assert lib.vk_debug_render_samples(ds._h, C.byref(cam), C.byref(q), img.ctypes.data, dump.ctypes.data) == ffi.VK_OK, lib.vk_last_error()
    return img, dump


def as_samples(states):
    res = np.zeros((len(states), 4), f32)
    res[:, :3] = states["acc"]
    res[:, 3] = np.ascontiguousarray(states["counter"]).view(f32)
    return res


def whole_frame(film, pb, q):
    film.emit(pb, 0, 0, q.width, q.height, 0, q.samples_per_pixel)
    assert pb.step(100000).live == 0
    film.deposit(pb)


# ---------------------------------------------------------------- 1. THE CONTRACT
@pytest.mark.parametrize("kind,name", S.ALL_SCENES, ids=[f"{k}-{n}" for k, n in S.ALL_SCENES])
def test_contract_on_scene(kind, name, device, host_scenes):
    desc, cam, p = S.scene(kind, name, host_scenes)
    W, H = p.width, p.height
    n = W * H * SPP
    ds = DeviceScene(desc)
    try:
        with ds.paths(n) as pb:
            for integrator in S.integrators(desc):
                for depth in S.DEPTHS:
                    what = f"{kind} {name}, integrator {integrator}, max_depth {depth}"
                    q = frame_params(p, integrator, SPP, depth)
                    _, dump = render_dump(ds, cam, q)
                    frame, stats = ds.render(cam, q)
                    with ds.film(cam, q) as film:
                        film.emit(pb, 0, 0, W, H, 0, SPP)
                        inf = pb.info()
                        assert inf.started == n and inf.live == n and inf.bounces == 0, what
                        assert pb.step(100000).live == 0, what
                        states, status = pb.results()
                        # 1. per id: that sample of vk_render
                        pixel, sample = F.ids_of(W, 0, 0, W, H, 0, SPP)
                        assert np.array_equal(states["pixel"], pixel) and np.array_equal(states["sample"], sample), what
                        assert (states["seed"] == q.seed).all() and np.isin(status, (ffi.VK_SHADE_MISS, ffi.VK_SHADE_ENDED)).all(), what
                        S.assert_samples_equal(as_samples(states), dump[F.dump_index(W, SPP, 0, 0, W, H, 0, SPP)], what)
                        # 2. the frame
                        film.deposit(pb)
                        want_sums, want_clamped = E.frame_sums(dump, W, H, SPP)
                        assert np.array_equal(film.debug_sums(), want_sums), what
                        assert np.array_equal(bits(film.resolve()), bits(frame)), what
                        finite = np.isfinite(dump[:, :3]).all(1)
                        inf = film.info()
                        assert (inf.width, inf.height, inf.samples_per_pixel) == (W, H, SPP), what
                        assert inf.dropped == int((~finite).sum()) and inf.clamped == stats.clamped_samples == want_clamped, what
                        assert inf.emitted == inf.deposited + inf.dropped == n and inf.skipped == 0 and inf.deposits == 1, what
                        ms = film.last_ms()
                        assert ms[0] > 0 and ms[1] > 0 and ms[2] > 0, what
    finally:
        ds.close()


# ---------------------------------------------------------------- 2. order and shapes
FW, FH = 40, 13
# (x0, y0, w, h, first_sample, n_samples): a partition of the 40 x 13 x 3 samples; path counts 259, 256, 40, 222, 63, 255, 65, 130, 50,
# 100, 1, 2, 32, 64, 21 — both sides of a wave (64) and of the compaction's workgroup (256) —, sample ranges split into [0,1) and [1,3)
# or taken whole, the [1,3) half of the first rectangle cut differently from its [0,1) half
WINDOWS = [(0, 0, 37, 7, 0, 1), (0, 0, 32, 4, 1, 2), (32, 0, 5, 4, 1, 2), (0, 4, 37, 3, 1, 2), (37, 0, 3, 7, 0, 3),
           (0, 7, 17, 5, 0, 3), (17, 7, 13, 5, 0, 1), (17, 7, 13, 5, 1, 2), (30, 7, 10, 5, 0, 1), (30, 7, 10, 5, 1, 2),
           (0, 12, 1, 1, 0, 1), (0, 12, 1, 1, 1, 2), (1, 12, 32, 1, 0, 1), (1, 12, 32, 1, 1, 2), (33, 12, 7, 1, 0, 3)]


def test_the_windows_partition_the_frame():
    seen = np.zeros(FW * FH * SPP, int)
    for w in WINDOWS:
        seen[F.dump_index(FW, SPP, *w)] += 1
    assert (seen == 1).all()
    counts = {w[2] * w[3] * w[5] for w in WINDOWS}
    assert {1, 63, 64, 65, 255, 256, 259} <= counts


def test_any_order_and_any_shapes_give_the_same_bytes(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    q = hs.params(FW, SPP, 20, seed=5, height=FH)
    ds = DeviceScene(hs.desc)
    multi = None
    try:
        frame, stats = ds.render(cam, q)
        with ds.film(cam, q) as one, ds.film(cam, q) as many, ds.paths(FW * FH * SPP) as big, ds.paths(259) as a, ds.paths(300) as b:
            whole_frame(one, big, q)
            order = np.random.default_rng(11).permutation(len(WINDOWS))
            for k, j in enumerate(order):
                pb = (a, b)[k % 2]
                w = WINDOWS[j]
                many.emit(pb, *w)
                assert pb.info().started == w[2] * w[3] * w[5]
                assert pb.step(100000).live == 0
                many.deposit(pb)
            assert many.debug_sums().tobytes() == one.debug_sums().tobytes()
            assert np.array_equal(bits(many.resolve()), bits(one.resolve())) and np.array_equal(bits(one.resolve()), bits(frame))
            i1, i2 = one.info(), many.info()
            assert (i2.emitted, i2.deposited, i2.dropped, i2.clamped, i2.skipped) == (i1.emitted, i1.deposited, i1.dropped, i1.clamped, i1.skipped)
            assert i2.deposits == len(WINDOWS) and i1.deposits == 1 and i1.clamped == stats.clamped_samples
            # 3. fewer samples than the film's: sample 0 of every pixel alone is vk_render's frame at one sample per pixel
            many.reset()
            assert not many.debug_sums().any() and many.info().emitted == 0 and many.info().deposits == 0
            for w in WINDOWS:
                if w[4] == 0:
                    many.emit(a, w[0], w[1], w[2], w[3], 0, 1)
                    a.step(100000)
                    many.deposit(a)
            first, _ = ds.render(cam, frame_params(q, spp=1))
            assert np.abs(first).max() < 1e9 and np.array_equal(bits(many.resolve(1)), bits(first))
        # the same frame on a multi-device scene (devices[0] does the work), through Film.render's own windows
        multi = DeviceScene(hs.desc, devices=[0, 0])
        with multi.film(cam, q) as film, multi.paths(200) as pb:
            assert np.array_equal(bits(film.render(pb)), bits(frame))
            assert film.info().deposits > 1 and film.info().emitted == FW * FH * SPP
    finally:
        if multi is not None:
            multi.close()
        ds.close()


# ---------------------------------------------------------------- 3. the deposit alone, both forms
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_deposit_alone_in_both_forms(n, device, host_scenes):
    """a batch begun with hand-made states and retired at once by vk_paths_cull(keep = 0): acc is exactly what the test wrote"""
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    W, H = 9, 5
    ds = DeviceScene(desc)
    try:
        rays = np.zeros(n, RAY_DTYPE)
        rays["direction"][:, 2], rays["tmax"] = -1.0, np.inf
        kw = S.shade_kwargs(p, p.integrator, 8)
        with ds.paths(n + 3) as pb:
            for spp in (3, 40):                              # 40: the clamp is 1.3e11 / 40, below 1e10
                q = frame_params(p, spp=spp)
                q.width, q.height = W, H
                with ds.film(cam, q) as film:
                    for name, pixel in F.pixel_patterns(n, W * H).items():
                        states = F.states_for(pixel, F.radiances(n, spp, seed=len(name)), seed=q.seed)
                        want, counters = F.deposit(states, np.full(n, ffi.VK_PATHS_CULLED, np.uint32), W, H, spp)
                        got = []
                        for form in FORMS:
                            film.reset()
                            film.debug_deposit_form(form)
                            pb.begin(rays, states, **kw)
                            pb.cull(np.zeros(n, np.uint8))
                            back, status = pb.results()
                            assert back.tobytes() == states.tobytes() and (status == ffi.VK_PATHS_CULLED).all()
                            film.deposit(pb)
                            what = f"n {n}, spp {spp}, {name}, form {form}"
                            sums = film.debug_sums()
                            assert np.array_equal(sums, want), what
                            assert F.counters_of(film.info()) == counters, (what, F.counters_of(film.info()), counters)
                            got.append(sums.tobytes())
                        assert got[0] == got[1], (n, spp, name)
                    if n == 257:
                        c = counters
                        assert c["dropped"] > 0 and c["clamped"] > 0 and c["skipped"] > 0 and c["deposited"] > 0
    finally:
        ds.close()


# ---------------------------------------------------------------- 4. a roulette between bounces
def test_roulette_between_bounces(device, host_scenes):
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    q = frame_params(p, max_depth=20)
    W, H = q.width, q.height
    ds = DeviceScene(desc)
    try:
        with ds.film(cam, q) as film, ds.paths(W * H * SPP) as pb:
            film.emit(pb, 0, 0, W, H, 0, SPP)
            pb.step(2)
            ids, _, live = pb.read()
            assert len(ids) > 64
            rng = np.random.default_rng(2)
            keep = (rng.random(len(ids)) < 0.75).astype(np.uint8)
            scale = np.full(len(ids), 1.0 / 0.75, f32)
            pb.cull(keep, scale)
            assert pb.step(100000).live == 0
            states, status = pb.results()
            gone = ids[keep == 0]
            assert len(gone) > 8 and (status[gone] == ffi.VK_PATHS_CULLED).all() and states[gone].tobytes() == live[keep == 0].tobytes()
            film.deposit(pb)
            want, counters = F.deposit(states, status, W, H, SPP)
            assert np.array_equal(film.debug_sums(), want) and F.counters_of(film.info()) == counters
            assert counters["skipped"] == 0 and counters["deposited"] + counters["dropped"] == W * H * SPP
            # and it is not the plain frame: the roulette changed samples
            plain, _ = ds.render(cam, q)
            assert not np.array_equal(bits(film.resolve()), bits(plain))
            # Film.render calls the rule between bounces, window after window; a rule that keeps every path leaves vk_render's frame
            calls = []

            def rule(b):
                calls.append(int(b.info().live))
                b.cull(np.ones(calls[-1], np.uint8))

            film.reset()
            with ds.paths(100) as small:
                assert np.array_equal(bits(film.render(small, cull=rule)), bits(plain))
            assert len(calls) > H and min(calls) >= 1 and film.info().deposits == H      # one row of all samples a window (72 paths fit 100, two rows do not)
    finally:
        ds.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_leave_film_and_batch_as_they_were(device, host_scenes):
    lib = device
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    q = frame_params(p, max_depth=8)
    W, H = q.width, q.height
    ds, other = DeviceScene(desc), DeviceScene(desc)
    try:
        # at create: vk_render's words, then the film's own four
        h = C.c_void_p(0x77)
        for change, word in ((dict(max_depth=0), b"max_depth must be >= 1"), (dict(tile_rank=1, tile_world=2), b"a film holds the whole image"),
                             (dict(output_format=ffi.VK_OUTPUT_RGB8), b"a film is f32 only"), (dict(width=1), b"width and height must be >= 2"),
                             (dict(samples_per_pixel=0), b"samples_per_pixel must be in 1..2^26"), (dict(width=8200, height=8200), b"width * height exceeds 2^26")):
            bad = ffi.RenderParams.from_buffer_copy(q)
            for k, v in change.items():
                setattr(bad, k, v)
            assert lib.vk_film_create(ds._h, C.byref(cam), C.byref(bad), C.byref(h)) == ffi.VK_ERR_BAD_ARG, word
            assert word in lib.vk_last_error(), lib.vk_last_error()
        assert h.value == 0x77
        with ds.film(cam, q) as film, ds.paths(W * H) as pb, other.paths(W * H) as foreign, ds.paths(16) as never:
            whole = lambda: film.emit(pb, 0, 0, W, H, 0, 1)
            whole()
            pb.step(1)
            sums0 = film.debug_sums().tobytes()

            def refused(call, word):
                before, fi = bytes(pb.info()), bytes(film.info())
                assert call() == ffi.VK_ERR_BAD_ARG, word
                assert word in lib.vk_last_error(), lib.vk_last_error()
                assert bytes(pb.info()) == before and bytes(film.info()) == fi and film.debug_sums().tobytes() == sums0, word

            emit = lambda b, *w: lib.vk_film_emit(film._h, b._h, C.byref(ffi.FilmWindow(*w)))
            assert pb.info().live > 0
            refused(lambda: lib.vk_film_deposit(film._h, pb._h), b"live paths (step or cull them first)")
            refused(lambda: emit(pb, W - 3, 0, 4, 2, 0, 1), b"outside the film's frame")
            refused(lambda: emit(pb, 0, H - 1, 2, 2, 0, 1), b"outside the film's frame")
            refused(lambda: emit(pb, 0xFFFFFFFF, 0, 2, 2, 0, 1), b"outside the film's frame")
            refused(lambda: emit(pb, 0, 0, 0, 2, 0, 1), b"empty window")
            refused(lambda: emit(pb, 0, 0, 2, 2, 0, 0), b"empty window")
            refused(lambda: emit(pb, 0, 0, 2, 2, SPP - 1, 2), b"exceeds the film's samples_per_pixel")
            refused(lambda: emit(pb, 0, 0, W, H, 0, 2), b"exceed the path batch's capacity")
            refused(lambda: emit(foreign, 0, 0, 2, 2, 0, 1), b"belongs to another scene")
            refused(lambda: lib.vk_film_deposit(film._h, foreign._h), b"belongs to another scene")
            refused(lambda: lib.vk_film_deposit(film._h, never._h), b"before vk_paths_begin or vk_film_emit")
            # the live batch is as it was: it finishes as a batch that was never bothered
            pb.step(100000)
            film.deposit(pb)
            sums0 = film.debug_sums().tobytes()
            assert film.info().deposits == 1
            refused(lambda: lib.vk_film_deposit(film._h, pb._h), b"deposited since its last begin or emit")
            # an emit, and a vk_paths_begin, clear the flag
            film.reset()
            whole()
            pb.step(100000)
            film.deposit(pb)
            assert film.debug_sums().tobytes() == sums0
            states, _ = pb.results()
            rays = np.zeros(len(states), RAY_DTYPE)
            pb.begin(rays, states, **S.shade_kwargs(q, q.integrator, 8))
            pb.cull(np.zeros(len(states), np.uint8))
            film.reset()
            film.deposit(pb)
            assert film.debug_sums().tobytes() == sums0
    finally:
        other.close()
        ds.close()


# ---------------------------------------------------------------- 6. scene state, lifecycle
def test_a_film_leaves_the_render_the_queries_and_a_progress_handle_alone(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    p = hs.params(96, 4, 20, seed=3)
    fq = hs.params(24, SPP, 20, seed=4, height=16)
    rays = S.rays_of(cam)
    ds = DeviceScene(hs.desc)
    try:
        before, _ = ds.render(cam, p)
        ms, requeued = ds.last_kernel_ms(), ds.last_requeued_samples()
        launches = [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)]
        hits = ds.trace_rays(rays, S.SEED, S.FIRST)
        with ds.film(cam, fq) as film, ds.paths(24 * 16 * SPP) as pb:
            whole_frame(film, pb, fq)
            first = film.debug_sums().copy()
            film.resolve()
            # (the same two events: HIP converts their ticks through a calibration that may move the answer by a nanosecond from call to
            # call; events recorded again would time another interval altogether)
            assert abs(ds.last_kernel_ms() - ms) < 1e-4 and ds.last_requeued_samples() == requeued
            assert [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)] == launches and launches
            after, _ = ds.render(cam, p)
            np.testing.assert_array_equal(bits(before), bits(after))
            np.testing.assert_array_equal(bits(ds.trace_rays(rays, S.SEED, S.FIRST)), bits(hits))
            film.reset()
            whole_frame(film, pb, fq)
            np.testing.assert_array_equal(film.debug_sums(), first)
            # a progress handle interrupted by a film frame is one that was not
            with ds.progress(cam, p) as pr:
                pr.step(2)
                moments = pr.moments()[0].copy()
                info = bytes(pr.info())
                film.reset()
                whole_frame(film, pb, fq)
                assert bytes(pr.info()) == info
                np.testing.assert_array_equal(pr.moments()[0], moments)
                interrupted, _ = pr.step(2)
            with ds.progress(cam, p) as pr:
                pr.step(2)
                plain, _ = pr.step(2)
            np.testing.assert_array_equal(bits(interrupted), bits(plain))
    finally:
        ds.close()


def test_two_films_alternately_reset_with_a_camera_and_destroy_null(device, host_scenes):
    hs, cam = host_scenes("final_scene")
    cam2 = ffi.Camera.from_buffer_copy(cam)
    cam2.origin[0] += 25.0
    qa = hs.params(24, SPP, 50, seed=6, height=16)
    qb = hs.params(17, 2, 12, seed=7, height=11)
    ds = DeviceScene(hs.desc)
    try:
        ds._lib.vk_film_destroy(None)
        want_a, _ = ds.render(cam, qa)
        want_b, _ = ds.render(cam2, qb)
        want_a2, _ = ds.render(cam2, qa)
        assert not np.array_equal(bits(want_a), bits(want_a2))
        with ds.film(cam, qa) as fa, ds.film(cam2, qb) as fb, ds.paths(24 * 16) as pa, ds.paths(17 * 11 + 5) as pb:
            # sample by sample, the two films and their batches interleaved bounce by bounce
            for s in range(SPP):
                fa.emit(pa, 0, 0, 24, 16, s, 1)
                if s < 2:
                    fb.emit(pb, 0, 0, 17, 11, s, 1)
                while pa.info().live or pb.info().live:
                    pa.step(1)
                    pb.step(2)
                fa.deposit(pa)
                if s < 2:
                    fb.deposit(pb)
            assert np.array_equal(bits(fa.resolve()), bits(want_a)) and np.array_equal(bits(fb.resolve()), bits(want_b))
            # vk_film_reset with a new camera equals a fresh film; without one it keeps the camera
            fa.reset(cam2)
            assert not fa.debug_sums().any() and bytes(fa.info())[16:] == bytes(48)
            assert np.array_equal(bits(fa.render(pa)), bits(want_a2))
            fa.reset()
            assert np.array_equal(bits(fa.render(pb)), bits(want_a2))
            bad = ffi.Camera.from_buffer_copy(cam)
            bad.time1 = bad.time0
            assert ds._lib.vk_film_reset(fa._h, C.byref(bad)) == ffi.VK_ERR_BAD_ARG and b"time0 >= time1" in ds._lib.vk_last_error()
            assert np.array_equal(bits(fa.resolve()), bits(want_a2))
    finally:
        ds.close()
