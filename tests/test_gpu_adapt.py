"""-m gpu: a film's error moments and adaptive regeneration (vk_adapt_*).  On the scenes and sizes of tests/test_gpu_adaptive.py (budget
64, windows of 8, its tolerance() recipe) the reference is a vk_progress handle of the same scene, camera and parameters:
  1. moments: whatever carried the samples — whole-frame regenerating runs, emit / deposit, tile runs; capacities 63 to 773; slicing by
     max_bounces 1 and 7 — vk_debug_adapt_moments is vk_debug_progress_moments and vk_adapt_stderr is vk_progress_stderr, bit for bit;
  2. decisions: with the same vk_adaptive_params the tile map after every close is the handle's after the same step and vk_adapt_resolve
     that step's image, bit for bit; every pixel is vk_render's at its tile's count;
  3. schedule: on a 21 x 13 frame with imposed tile maps, vk_paths_read after every bounce of a tile run is tests/regen_ref.py's
     schedule() with the ids of tests/adapt_ref.py's sequence, and vk_debug_adapt_sequence is that enumeration;
then a map with no tile active, a roulette rule with a cull between steps, the refusals, and the absence of side effects.  The
mixed-tiles condition (0 < tiles_active < tiles_total) is asserted on the vk_progress reference's map, never on the film's."""
import ctypes as C

import numpy as np
import pytest

import adapt_ref as A
import regen_ref as G
import test_gpu_adaptive as GA
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu

SCENES, BUDGET, WINDOW = GA.SCENES, GA.BUDGET, GA.WINDOW
STEPS = BUDGET // WINDOW
bits = GA.bits
ALL = 0xFFFFFFFF


def finished(info):
    return info.live == 0 and info.remaining == 0


def run_to_end(film, pb, max_bounces=ALL):
    while not finished(film.regen_step(pb, max_bounces)):
        pass


_refs = {}


def reference(name, width, adaptive):
    """the vk_progress handle's record after every step, computed once: moments, tile map, image; and its stderr after the last"""
    key = (name, width, adaptive)
    if key not in _refs:
        hs, cam, ds = GA.scene(name, width)
        p = hs.params(width, BUDGET, 50)
        ap = GA.adaptive(name, width) if adaptive else None
        steps = []
        with ds.progress(cam, p, stderr=True, adaptive=ap) as pr:
            for _ in range(STEPS):
                img, _ = pr.step(WINDOW)
                run, m2 = pr.moments()
                tmap, inf = pr.tile_samples()
                steps.append(dict(img=img.copy(), run=run.copy(), m2=m2.copy(), tmap=tmap.copy(), active=inf.tiles_active,
                                  rendered=inf.samples_rendered))
            se = pr.stderr()
            assert pr.info().clamped_samples == 0
        _refs[key] = (steps, se, ap)
    return _refs[key]


def same_moments(film, step, what):
    run, m2 = film.debug_moments()
    assert run.tobytes() == step["run"].tobytes(), f"{what}: the sums differ from the vk_progress handle's"
    assert m2.tobytes() == step["m2"].tobytes(), f"{what}: the moments differ from the vk_progress handle's"


# ---------------------------------------------------------------- 1. moments, whatever carried the samples
# per window: the route, the batch's capacity, max_bounces
ROUTES = [("frame run", 63, 1), ("emit", None, None), ("frame run", 64, 7), ("tile run", 65, 7), ("frame run", 257, 1), ("emit", None, None),
          ("frame run", 773, 7), ("tile run", 257, 1)]


@pytest.mark.parametrize("name,width", SCENES)
def test_moments_are_the_progress_handles(name, width, device):
    hs, cam, ds = GA.scene(name, width)
    p = hs.params(width, BUDGET, 50)
    steps, want_se, _ = reference(name, width, False)
    W, H = p.width, p.height
    assert len(ROUTES) == STEPS and {c for _, c, _ in ROUTES if c} == {63, 64, 65, 257, 773}
    batches = {c: ds.paths(c) for c in {c for _, c, _ in ROUTES if c}}
    try:
        with ds.film(cam, p) as film, ds.paths(W * H * WINDOW) as big:
            film.enable_adaptive()                                      # moments only
            for j, (route, cap, mb) in enumerate(ROUTES):
                what = f"{name}, window {j} by {route}, capacity {cap}, max_bounces {mb}"
                if route == "frame run":
                    film.regen_begin(batches[cap], 0, 0, W, H, j * WINDOW, WINDOW)
                    run_to_end(film, batches[cap], mb)
                elif route == "tile run":
                    film.adapt_begin(batches[cap], WINDOW)
                    assert batches[cap].info().live == 0 and batches[cap].info().started == 0
                    run_to_end(film, batches[cap], mb)
                    assert batches[cap].info().started == W * H * WINDOW, what
                else:
                    film.emit(big, 0, 0, W, H, j * WINDOW, WINDOW)
                    assert big.step(100000).live == 0
                    film.deposit(big)
                info = film.adapt_close(WINDOW)
                assert (info.samples_done, info.steps) == ((j + 1) * WINDOW, j + 1), what
                assert info.tiles_active == info.tiles_total == steps[j]["tmap"].size and info.pixels_active == W * H, what
                assert info.samples_rendered == W * H * (j + 1) * WINDOW, what
                same_moments(film, steps[j], what)
                assert np.array_equal(bits(film.resolve_adaptive()), bits(steps[j]["img"])), what
            se = film.stderr()
            assert np.array_equal(bits(se), bits(want_se)), f"{name}: {int((se != want_se).sum())} components of the standard error differ"
            assert np.array_equal(bits(film.resolve(BUDGET)), bits(steps[-1]["img"]))
            assert film.info().clamped == 0
    finally:
        for b in batches.values():
            b.close()


# ---------------------------------------------------------------- 2. decisions
@pytest.mark.parametrize("name,width", SCENES)
def test_decisions_are_the_progress_handles(name, width, device):
    hs, cam, ds = GA.scene(name, width)
    p = hs.params(width, BUDGET, 50)
    steps, want_se, ap = reference(name, width, True)
    last = steps[-1]
    assert 0 < last["active"] < last["tmap"].size, "the inputs: the reference run must end with mixed tiles"
    px = A.tile_pixels(p.width, p.height)
    with ds.film(cam, p) as film, ds.paths(4099) as pb:
        film.enable_adaptive(**ap)
        emitted = 0
        for j, step in enumerate(steps):
            what = f"{name}, close {j}"
            # (the reference's own record says which tiles a window rendered: those whose count it moved)
            was_active = step["tmap"] > steps[j - 1]["tmap"] if j else np.ones(step["tmap"].shape, bool)
            film.adapt_begin(pb, WINDOW)
            run_to_end(film, pb, 7 if j % 2 else ALL)
            emitted += int((px * was_active).sum()) * WINDOW
            assert pb.info().started == int((px * was_active).sum()) * WINDOW and film.info().emitted == emitted, what
            info = film.adapt_close(WINDOW)
            tmap, inf = film.tile_samples()
            assert np.array_equal(tmap, step["tmap"]), f"{what}: the tile maps differ"
            assert info.tiles_active == inf.tiles_active == step["active"] and info.tiles_total == inf.tiles_total == tmap.size, what
            assert info.samples_rendered == inf.samples_rendered == step["rendered"] == emitted, what
            if j + 1 < STEPS:
                assert info.pixels_active == int((px * (steps[j + 1]["tmap"] > step["tmap"])).sum()), what
            same_moments(film, step, what)
            assert np.array_equal(bits(film.resolve_adaptive()), bits(step["img"])), f"{what}: the images differ"
        assert np.array_equal(bits(film.stderr()), bits(want_se)), name
        GA.check_exact(ds, cam, p, film.resolve_adaptive(), tmap)
        fi = film.info()
        assert fi.emitted == fi.deposited + fi.dropped + fi.skipped == emitted and fi.clamped == 0


# ---------------------------------------------------------------- 3. the schedule of a tile run, on imposed maps
W3, H3, N3, DEPTH3 = 21, 13, 2, 12


@pytest.fixture(scope="module")
def frame3(device, host_scenes):
    """the 21 x 13 frame stepped whole by the window route, one bounce a call: per frame id (pixel * N3 + k) the lifetime and, per age,
    the ray and the state; and the sums the whole window leaves"""
    hs, cam = host_scenes("cornell_box")
    p = hs.params(W3, 16, DEPTH3, seed=5, height=H3)
    ds = DeviceScene(hs.desc)
    total = W3 * H3 * N3
    with ds.film(cam, p) as ref, ds.paths(total) as big:
        ref.emit(big, 0, 0, W3, H3, 0, N3)
        hist = [big.read()]
        while big.info().live:
            big.step(1)
            hist.append(big.read())
        ref.deposit(big)
        sums = ref.debug_sums().copy()
    ids_at = [h[0] for h in hist]
    life = G.lifetimes_of(ids_at, total)
    rays_at = np.stack(G.by_id(ids_at, [h[1] for h in hist], total))
    states_at = np.stack(G.by_id(ids_at, [h[2] for h in hist], total))
    assert life.max() > 2
    yield ds, cam, p, life, rays_at, states_at, sums
    ds.close()


@pytest.mark.parametrize("which", ["all active", "checkerboard", "top-right only", "tile 0 frozen"])
def test_every_bounce_of_a_tile_run_is_the_schedule(which, frame3):
    ds, cam, p, life, rays_at, states_at, frame_sums = frame3
    tile_n = A.tile_maps(W3, H3)[which]
    pixel, sample = A.sequence(W3, H3, tile_n, N3)
    at = pixel.astype(np.int64) * N3 + sample                       # the run's id -> the frame's
    total = len(pixel)
    act = A.active_mask(W3, H3, tile_n)
    assert total == int(act.sum()) * N3 > 0
    with ds.film(cam, p) as film:
        film.enable_adaptive()
        film.debug_set_tiles(tile_n)
        # the top-up kernel's index code against the enumeration: every q, and a range that starts inside a tile
        got = film.debug_sequence(N3, 0, total)
        assert np.array_equal(got[0], pixel) and np.array_equal(got[1], sample), which
        first = 5 * N3 + 1
        got = film.debug_sequence(N3, first, total - first - 2)
        assert np.array_equal(got[0], pixel[first:-2]) and np.array_equal(got[1], sample[first:-2]), which
        tmap, inf = film.tile_samples()
        assert inf.tiles_active == int((tile_n == 0).sum()) and np.array_equal(tmap, tile_n)
        run_life = life[at]
        for cap in (1, 64, 65, total + 7):
            sched = G.schedule(run_life, cap)
            film.reset()
            film.debug_set_tiles(tile_n)
            with ds.paths(cap) as pb:
                film.adapt_begin(pb, N3)
                assert pb.info().live == 0 and pb.info().started == 0 and len(pb.read()[0]) == 0
                for k, b in enumerate(sched):
                    what = f"{which}, capacity {cap}, bounce {k}"
                    info = film.regen_step(pb, 1)
                    assert info.bounces == 1 and info.traced == len(b["before"]) and info.live == len(b["after"]), what
                    assert info.emitted == int((b["before_age"] == 0).sum()) and info.kernel_launches == (6 if info.emitted else 5), what
                    ids, rays, states = pb.read()
                    assert np.array_equal(ids, b["after"]), what
                    want_r, want_s = rays_at[b["after_age"], at[b["after"]]], states_at[b["after_age"], at[b["after"]]]
                    assert rays.tobytes() == want_r.tobytes() and states.tobytes() == want_s.tobytes(), what
                    assert finished(info) == (k == len(sched) - 1), what
                assert pb.info().bounces == len(sched) and pb.info().started == total
                if cap == 64:
                    ms = film.regen_last_ms(pb)
                    assert len(ms) == 4 and min(ms) >= 0 and ms[1] > 0
            # what the run deposited: the whole window's sums in the active tiles, nothing elsewhere
            sums = film.debug_sums()
            assert np.array_equal(sums[act], frame_sums[act]) and not sums[~act].any(), (which, cap)
            info = film.adapt_close(N3)
            assert info.samples_done == N3 and info.samples_rendered == int((tile_n * A.tile_pixels(W3, H3)).sum()) + total
            run, m2 = film.debug_moments()
            want_prev, want_m2 = A.fold(sums, np.zeros_like(sums), np.zeros(sums.shape), tile_n, N3)
            assert run.tobytes() == want_prev.tobytes() and m2.tobytes() == want_m2.tobytes(), (which, cap)


# ---------------------------------------------------------------- 4. no tile active
def test_no_tile_active(frame3):
    ds, cam, p = frame3[:3]
    with ds.film(cam, p) as film, ds.paths(100) as pb:
        film.enable_adaptive()
        for _ in range(2):
            film.adapt_begin(pb, 3)
            run_to_end(film, pb)
            film.adapt_close(3)
        img, se = film.resolve_adaptive().copy(), film.stderr().copy()
        moments = [a.tobytes() for a in film.debug_moments()]
        tx, ty = A.tile_grid(W3, H3)
        film.debug_set_tiles(np.full((ty, tx), 6, np.uint32), np.full((ty, tx), 2, np.uint32))
        emitted = film.info().emitted
        film.adapt_begin(pb, 4)                                         # a finished run
        pi = pb.info()
        assert pi.live == 0 and pi.started == 0 and len(pb.read()[0]) == 0
        info = film.regen_step(pb, 5)
        assert finished(info) and info.bounces == 0 and info.kernel_launches == 0 and film.info().emitted == emitted
        info = film.adapt_close(4)                                      # the counts advance, no tile changes
        assert (info.samples_done, info.steps, info.tiles_active, info.pixels_active) == (10, 3, 0, 0)
        assert info.samples_rendered == W3 * H3 * 6
        tmap, inf = film.tile_samples()
        assert (tmap == 6).all() and inf.tiles_active == 0 and inf.samples_rendered == W3 * H3 * 6
        assert np.array_equal(bits(film.resolve_adaptive()), bits(img)) and np.array_equal(bits(film.stderr()), bits(se))
        assert [a.tobytes() for a in film.debug_moments()] == moments
        # vk_film_reset: every tile active again, sample 0
        film.reset()
        tmap, inf = film.tile_samples()
        assert not tmap.any() and inf.tiles_active == inf.tiles_total and not film.debug_moments()[0].any() and not film.debug_moments()[1].any()
        assert film.adapt_close(1).samples_done == 1


# ---------------------------------------------------------------- 5. with a roulette rule and a cull between steps
def test_runs_finish_under_a_rule_and_a_cull(device):
    name, width = "cornell_box", 48
    hs, cam, ds = GA.scene(name, width)
    p = hs.params(width, BUDGET, 50)
    px = A.tile_pixels(p.width, p.height)
    with ds.film(cam, p) as film, ds.paths(1500) as pb:
        film.enable_adaptive(**GA.adaptive(name, width))
        pb.set_roulette(3, 0.05, 0.9)
        calls = [0]

        def cull(batch):
            calls[0] += 1
            ids = batch.read()[0]
            film.regen_cull(batch, (ids % 7 != 3) | (calls[0] % 3 != 0))
        img, info = film.render_adaptive(pb, WINDOW, cull=cull)
        assert calls[0] > 10 and pb.info().live == 0 and pb.info().retired[4] > 0
        tmap, inf = film.tile_samples()
        assert info.samples_done <= BUDGET and info.samples_done == info.steps * WINDOW
        assert ((tmap % WINDOW) == 0).all() and tmap.max() == info.samples_done and tmap.min() >= 2 * WINDOW
        assert inf.tiles_active == info.tiles_active <= int((tmap == info.samples_done).sum())
        fi = film.info()
        assert fi.emitted == fi.deposited + fi.dropped + fi.skipped
        assert fi.emitted == inf.samples_rendered == info.samples_rendered == int((tmap.astype(np.int64) * px).sum())
        assert np.isfinite(img).all() and np.array_equal(bits(img), bits(film.resolve_adaptive()))


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_film_batch_and_moments_as_they_were(device, host_scenes):
    name, width = "cornell_box", 48
    hs, cam, ds = GA.scene(name, width)
    p = hs.params(width, BUDGET, 50)
    lib = ds._lib
    hs2, _ = host_scenes("final_scene")
    other = DeviceScene(hs2.desc)
    try:
        with ds.film(cam, p) as film, ds.film(cam, p) as plain, ds.film(cam, hs.params(width, 1 << 26, 50)) as huge, \
                ds.paths(300) as pb, other.paths(8) as foreign:
            film.enable_adaptive(**GA.adaptive(name, width))
            huge.enable_adaptive()
            film.adapt_begin(pb, WINDOW)
            film.regen_step(pb, 2)
            run_to_end(film, pb)
            film.adapt_close(WINDOW)
            film.regen_begin(pb, 0, 0, 4, 4, WINDOW, 1)
            film.regen_step(pb, 1)                                      # a batch in the middle of a run
            assert pb.info().live > 0
            info, img = ffi.AdaptInfo(9, 9, 9, 9, 9, 9), np.full((p.height, p.width, 3), 7, np.float32)
            ok = ffi.AdaptiveParams(1e-3, 0.0, 0, 2)

            def refused(call, word):
                state = lambda: ([bytes(x.info()) for x in (pb, film, plain, huge)], [a.tobytes() for a in film.debug_moments()],
                                 film.tile_samples()[0].tobytes(), bytes(film.tile_samples()[1]))
                before = state()
                assert call() == ffi.VK_ERR_BAD_ARG, word
                assert word in lib.vk_last_error(), lib.vk_last_error()
                assert state() == before, word
                assert bytes(info) == bytes(ffi.AdaptInfo(9, 9, 9, 9, 9, 9)) and (img == 7).all()

            refused(lambda: lib.vk_adapt_enable(film._h, C.byref(ok)), b"before the film's first emit or deposit")
            refused(lambda: lib.vk_adapt_enable(film._h, None), b"before the film's first emit or deposit")
            refused(lambda: lib.vk_adapt_enable(plain._h, C.byref(ffi.AdaptiveParams(1e-3, 0.0, 0, 1))), b"min_steps must be >= 2")
            refused(lambda: lib.vk_adapt_begin(None, pb._h, 1), b"null argument")
            refused(lambda: lib.vk_adapt_begin(film._h, None, 1), b"null argument")
            refused(lambda: lib.vk_adapt_begin(plain._h, pb._h, 1), b"without vk_adapt_enable")
            refused(lambda: lib.vk_adapt_begin(film._h, pb._h, 0), b"n_samples must be >= 1")
            refused(lambda: lib.vk_adapt_begin(film._h, pb._h, BUDGET - WINDOW + 1), b"exceeds the film's samples_per_pixel")
            refused(lambda: lib.vk_adapt_begin(film._h, foreign._h, 1), b"belongs to another scene")
            refused(lambda: lib.vk_adapt_begin(huge._h, pb._h, 1 << 26), b"exceed 2^32 - 1")
            refused(lambda: lib.vk_adapt_close(None, 1, C.byref(info)), b"null film")
            refused(lambda: lib.vk_adapt_close(plain._h, 1, C.byref(info)), b"without vk_adapt_enable")
            refused(lambda: lib.vk_adapt_close(film._h, 0, C.byref(info)), b"n_samples must be >= 1")
            refused(lambda: lib.vk_adapt_close(film._h, BUDGET - WINDOW + 1, C.byref(info)), b"exceeds the film's samples_per_pixel")
            refused(lambda: lib.vk_adapt_resolve(plain._h, img.ctypes.data), b"without vk_adapt_enable")
            refused(lambda: lib.vk_adapt_resolve(huge._h, img.ctypes.data), b"before the first vk_adapt_close")
            refused(lambda: lib.vk_adapt_resolve(film._h, None), b"null argument")
            refused(lambda: lib.vk_adapt_stderr(plain._h, img.ctypes.data), b"without vk_adapt_enable")
            refused(lambda: lib.vk_adapt_stderr(film._h, img.ctypes.data), b"needs two closes or more")
            refused(lambda: lib.vk_adapt_tile_samples(plain._h, None, None), b"without vk_adapt_enable")
            refused(lambda: lib.vk_debug_adapt_moments(plain._h, None, None), b"without vk_adapt_enable")
            seq = np.full(8, 7, np.uint32)
            refused(lambda: lib.vk_debug_adapt_sequence(film._h, 0, 0, 4, seq.ctypes.data, seq.ctypes.data), b"n_samples must be >= 1")
            refused(lambda: lib.vk_debug_adapt_sequence(film._h, 1, p.width * p.height - 2, 4, seq.ctypes.data, seq.ctypes.data), b"beyond the tile run")
            assert (seq == 7).all()
            # the interrupted run goes on as if nothing had been asked
            run_to_end(film, pb)
            # called again before the first emit, vk_adapt_enable takes the new parameters; after a reset it may be called again
            assert lib.vk_adapt_enable(huge._h, C.byref(ok)) == ffi.VK_OK and lib.vk_adapt_enable(huge._h, None) == ffi.VK_OK
            film.reset()
            assert lib.vk_adapt_enable(film._h, C.byref(ok)) == ffi.VK_OK
    finally:
        other.close()


# ---------------------------------------------------------------- 7. no side effect
def test_nothing_else_is_touched(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    p = hs.params(96, 4, 20, seed=3)
    fq = hs.params(24, 12, 20, seed=4, height=16)
    ds = DeviceScene(hs.desc)
    multi = None
    try:
        with ds.film(cam, fq) as film, ds.paths(100) as pb, ds.progress(cam, p, stderr=True) as pr:
            pr.step(2)                                                  # a live vk_progress handle
            moments = [a.copy() for a in pr.moments()]
            info = bytes(pr.info())
            before, _ = ds.render(cam, p)
            ms, requeued = ds.last_kernel_ms(), ds.last_requeued_samples()
            launches = [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)]
            film.enable_adaptive(abs_tol=0.05, min_steps=2)
            img, last = film.render_adaptive(pb, 4)
            assert last.samples_done == 12 or last.tiles_active == 0
            assert abs(ds.last_kernel_ms() - ms) < 1e-4 and ds.last_requeued_samples() == requeued
            assert [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)] == launches and launches
            after, _ = ds.render(cam, p)
            np.testing.assert_array_equal(bits(before), bits(after))
            assert bytes(pr.info()) == info
            for a, b in zip(pr.moments(), moments):
                np.testing.assert_array_equal(a, b)
            tmap = film.tile_samples()[0]
            GA.check_exact(ds, cam, fq, img, tmap)
            # a film without vk_adapt_enable: vk_render's frame and the counters of a regenerating frame
            frame, _ = ds.render(cam, fq)
            with ds.film(cam, fq) as plain:
                assert np.array_equal(bits(plain.render_regen(pb)), bits(frame))
                fi = plain.info()
                assert fi.deposits == 0 and fi.emitted == 24 * 16 * 12 == fi.deposited + fi.dropped + fi.skipped
                assert ds._lib.vk_adapt_close(plain._h, 1, None) == ffi.VK_ERR_BAD_ARG
        # a multi-device scene: devices[0] does the work, the same decisions and the same image
        multi = DeviceScene(hs.desc, devices=[0, 0])
        with multi.film(cam, fq) as film, multi.paths(200) as pb:
            film.enable_adaptive(abs_tol=0.05, min_steps=2)
            got, _ = film.render_adaptive(pb, 4)
            assert np.array_equal(bits(got), bits(img)) and np.array_equal(film.tile_samples()[0], tmap)
    finally:
        if multi is not None:
            multi.close()
        ds.close()
