"""Robust film on the device.  FILM PARITY: a film's camera paths deposited into accumulators of 2, 5, 8 and 16 buckets next to the film
itself — the raw state is tests/robust_ref.py's restatement of the batches' results, the buckets add up to the film's sums, the counters
are the film's, and MEAN is vk_film_resolve's and vk_render's frame, bit for bit, however the frame was cut into windows.  On those
states the TRIM and GINI images and the standard error equal the restatement.  The deposit alone on injected results: one firefly, a
NaN, a pixel outside the frame, a component beyond the clamp, batch lengths on both sides of a wave and of a workgroup.  Flags, the six
orders of film, splat and robust deposits, reset, refusals."""
import ctypes as C
import itertools

import numpy as np
import pytest

import film_ref as F
import robust_ref as R
import shade_ref as S
from vecchio_amd import DeviceScene, ffi
from vecchio_amd.scene import RAY_DTYPE

pytestmark = pytest.mark.gpu
f32 = np.float32
SPP = 12
FRAMES = [(24, 16), (33, 17)]
BUCKETS = (2, 5, 8, 16)                      # 12 samples: 5 gives unequal counts, 16 empty buckets
SCENES = [("builder", "cornell_box", ffi.VK_INTEGRATOR_PDF), ("special", "media_and_textures", ffi.VK_INTEGRATOR_PDF),
          ("special", "scatter_sky", ffi.VK_INTEGRATOR_SCATTER)]
HOWS = [(R.MEAN, 0), (R.TRIM, 1), (R.TRIM, 2), (R.TRIM, 0xFFFFFFFF), (R.GINI, 0)]
LENGTHS = (1, 63, 64, 65, 255, 256, 257)     # wave and workgroup boundaries


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frame_params(p, W, H, integrator, spp=SPP):
    q = ffi.RenderParams.from_buffer_copy(p)
    q.width, q.height, q.samples_per_pixel, q.integrator = W, H, spp, integrator
    q.max_depth = min(int(p.max_depth), 12)
    return q


def cut(x0, y0, w, h, cap, ns, spp=SPP):
    """Film.windows()'s walk, of the block (x0, y0, w, h) of the frame in sample chunks of ns, for a batch of `cap` paths"""
    assert ns <= cap
    ww = max(1, min(w, cap // ns))
    hh = max(1, min(h, cap // (ns * ww)))
    for s0 in range(0, spp, ns):
        for yy in range(y0, y0 + h, hh):
            for xx in range(x0, x0 + w, ww):
                yield xx, yy, min(ww, x0 + w - xx), min(hh, y0 + h - yy), s0, min(ns, spp - s0)


def windows_of(W, H):
    """a partition of the W x H x 12 samples: capacities 1, 63, 64, 65, 255, 256 and 257 cutting their blocks into windows of 1, 4 and
    12 samples per pixel — with 4 and 12 a wave holds several samples of one bucket for K = 2"""
    blocks = [((0, 0, 3, 1), 1, 1), ((3, 0, W - 3, 1), 64, 4), ((0, 1, W, 3), 63, 1), ((0, 4, W, 3), 65, 4), ((0, 7, W, 3), 255, 12),
              ((0, 10, W, 3), 256, 4), ((0, 13, W, H - 13), 257, 12)]
    out = []
    for rect, cap, ns in blocks:
        out += [(win, cap) for win in cut(*rect, cap, ns)]
    return out


def test_the_windows_partition_the_frames():
    for W, H in FRAMES:
        seen = np.zeros(W * H * SPP, int)
        wins = windows_of(W, H)
        for win, cap in wins:
            assert win[2] * win[3] * win[5] <= cap
            seen[F.dump_index(W, SPP, *win)] += 1
        assert (seen == 1).all()
        assert {1, 4, 12} <= {win[5] for win, _ in wins} and {1, 63, 64, 65, 255, 256, 257} == {cap for _, cap in wins}


# ---------------------------------------------------------------- 1. film parity, 2. resolve
@pytest.mark.parametrize("frame", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
@pytest.mark.parametrize("kind,name,integrator", SCENES, ids=[s[1] for s in SCENES])
def test_film_parity_and_resolve(kind, name, integrator, frame, device, host_scenes):
    desc, cam, p = S.scene(kind, name, host_scenes)
    assert integrator in S.integrators(desc)
    W, H = frame
    q = frame_params(p, W, H, integrator)
    wins = windows_of(W, H)
    ds = DeviceScene(desc)
    try:
        render, _ = ds.render(cam, q)
        accs = [ds.robust(W, H, SPP, buckets=K, mode=ffi.VK_ROBUST_MEAN) for K in BUCKETS]
        batches = {cap: ds.paths(cap) for cap in sorted({cap for _, cap in wins})}
        want = [np.zeros((H, W, K, 4), np.int64) for K in BUCKETS]
        counters = dict.fromkeys(R.COUNTERS, 0)
        try:
            with ds.film(cam, q) as film:
                for j in np.random.default_rng(W).permutation(len(wins)):
                    win, cap = wins[j]
                    pb = batches[cap]
                    # (a batch goes into ONE robust accumulator per emit: the window is emitted again for each, and gives the same results)
                    for i, acc in enumerate(accs):
                        film.emit(pb, *win)
                        assert pb.step(100000).live == 0
                        if i == 0:
                            film.deposit(pb)
                            states, status = pb.results()
                        elif i == 1:
                            again = pb.results()
                            assert again[0].tobytes() == states.tobytes() and again[1].tobytes() == status.tobytes()
                        acc.deposit(pb)
                    for i, K in enumerate(BUCKETS):
                        want[i], c = R.deposit(states, status, W, H, SPP, K, want[i])
                    for k in counters:
                        counters[k] += c[k]
                film_sums, fi = film.debug_sums(), film.info()
                film_img = film.resolve(SPP)
                assert np.array_equal(bits(film_img), bits(render))
                for K, acc, w in zip(BUCKETS, accs, want):
                    what = f"{name} {W}x{H} K {K}"
                    state = acc.debug_sums()
                    assert state.shape == (H, W, K, 4) and np.array_equal(state, w), what
                    assert np.array_equal(state[..., :3].sum(axis=2), film_sums), what
                    assert (state[..., 3].sum(axis=2) == SPP).all(), what
                    ai = acc.info()
                    assert R.counters_of(ai) == F.counters_of(fi) == counters, what
                    assert (ai.width, ai.height, ai.samples_per_pixel, ai.buckets, ai.deposits) == (W, H, SPP, K, len(wins)), what
                    assert ((state[..., 3] > 0).sum(axis=2) == min(K, SPP)).all(), what
                    mean = acc.resolve()
                    assert np.array_equal(bits(mean), bits(film_img)) and np.array_equal(bits(mean), bits(render)), what
                    ms = acc.last_ms()
                    assert ms[0] > 0 and ms[1] > 0
                    # 2. every way to resolve, from `how` and from an accumulator created that way
                    for mode, trim in HOWS:
                        ref_rgb, ref_se = R.resolve(state, mode, trim)
                        rgb, se = acc.resolve(mode=mode, trim=trim, want_stderr=True)
                        assert np.array_equal(bits(rgb), bits(ref_rgb)) and np.array_equal(bits(se), bits(ref_se)), (what, mode, trim)
                        assert np.array_equal(bits(acc.resolve(mode=mode, trim=trim)), bits(rgb)), (what, mode, trim)
                    assert np.array_equal(acc.debug_sums(), state), what          # the sums stay
                # created with a `how`: the last window's batch alone, into accumulators of each mode
                states, status = pb.results()
                for mode, trim in HOWS[1:]:
                    with ds.robust(W, H, SPP, buckets=5, mode=mode, trim=trim) as own, \
                            ds.robust(W, H, SPP, buckets=5, mode=ffi.VK_ROBUST_MEAN) as plain:
                        film.emit(pb, *win)
                        assert pb.step(100000).live == 0
                        own.deposit(pb)
                        film.emit(pb, *win)
                        assert pb.step(100000).live == 0
                        plain.deposit(pb)
                        a, ae = own.resolve(want_stderr=True)
                        b, be = plain.resolve(mode=mode, trim=trim, want_stderr=True)
                        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(ae), bits(be)), (mode, trim)
                        assert np.array_equal(own.debug_sums(), R.deposit(states, status, W, H, SPP, 5)[0])
        finally:
            for acc in accs:
                acc.close()
            for pb in batches.values():
                pb.close()
    finally:
        ds.close()


# ---------------------------------------------------------------- 3. injected results
def dead_rays(n):
    rays = np.zeros(n, RAY_DTYPE)
    rays["direction"][:, 2], rays["tmax"] = -1.0, np.inf
    return rays


def stage(pb, states, kw):
    """a finished batch whose results are exactly `states`, every status VK_PATHS_CULLED: begun and retired at once (the way
    tests/test_gpu_splat.py stages its deposit batches)"""
    n = len(states)
    pb.begin(dead_rays(n), states, **kw)
    pb.cull(np.zeros(n, np.uint8))
    return np.full(n, ffi.VK_PATHS_CULLED, np.uint32)


def sums_between_canaries(acc):
    """vk_debug_robust_sums into the middle of a larger array: (the state, whether the rows around it are untouched)"""
    H, W, K = acc.height, acc.width, acc.buckets
    buf = np.full((H + 4, W, K, 4), 0x5A5A5A5A5A5A5A5A, np.int64)
    assert acc._lib.vk_debug_robust_sums(acc._h, buf[2:].ctypes.data) == ffi.VK_OK
    return buf[2:H + 2].copy(), bool((buf[:2] == 0x5A5A5A5A5A5A5A5A).all() and (buf[H + 2:] == 0x5A5A5A5A5A5A5A5A).all())


def test_injected_results(device, host_scenes):
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    W, H, K = 24, 16, 8
    kw = S.shade_kwargs(p, p.integrator, 8)
    clampv = float(R.E.accum_clamp_for(SPP))
    ds = DeviceScene(desc)
    try:
        with ds.paths(max(LENGTHS)) as pb, ds.robust(W, H, SPP, buckets=K) as acc:
            # one pixel's twelve samples and its neighbours': ordinary values, one 1e6 sample
            px = 5 * W + 7
            pixel = np.repeat(np.array([px - 1, px, px + 1, px - W, px + W], np.uint32), SPP)
            sample = np.tile(np.arange(SPP, dtype=np.uint32), 5)
            accv = (np.random.default_rng(2).random((len(pixel), 3)) * 0.5 + 0.25).astype(f32)
            spike = SPP + 6                                       # sample 6 of pixel px
            accv[spike] = (1e6, 1e6, 1e6)
            states = F.states_for(pixel, accv, seed=p.seed)
            states["sample"] = sample
            status = stage(pb, states, kw)
            acc.deposit(pb)
            want, counters = R.deposit(states, status, W, H, SPP, K)
            state, clean = sums_between_canaries(acc)
            assert clean and np.array_equal(state, want) and R.counters_of(acc.info()) == counters
            assert counters == dict(deposited=60, dropped=0, clamped=0, skipped=0)
            gini, se = acc.resolve(want_stderr=True)
            ref, ref_se, j, t, G = R.resolve(state, R.GINI, details=True)
            assert np.array_equal(bits(gini), bits(ref)) and np.array_equal(bits(se), bits(ref_se))
            y, x = divmod(px, W)
            assert t[y, x] == 3 and gini[y, x].max() < 1.0 and acc.resolve(mode=R.MEAN)[y, x].min() > 8e4
            # the neighbours are what they are without the spike, and the rest of the frame is black
            calm = accv.copy()
            calm[spike] = 0.5
            quiet = F.states_for(pixel, calm, seed=p.seed)
            quiet["sample"] = sample
            ref_quiet = R.resolve(R.deposit(quiet, status, W, H, SPP, K)[0], R.GINI)[0]
            others = np.ones((H, W), bool)
            others[y, x] = False
            assert np.array_equal(bits(gini[others]), bits(ref_quiet[others]))
            lit = np.zeros((H, W), bool)
            lit.reshape(-1)[np.unique(pixel)] = True
            assert not gini[~lit].any() and not se[~lit].any() and gini[lit].all()

            # a NaN (dropped, counted in its bucket), a pixel at width * height (skipped: nothing touched), components at and beyond
            # 31.999 and beyond the clamp (clamped), infinities; every one a culled path
            acc.reset()
            special = np.array([(np.nan, 0.5, 0.5), (0.5, 0.5, 0.5), (31.999, -31.999, 1.0), (float(np.nextafter(f32(31.999), f32(40))), 1, 2),
                                (clampv * 2, 1.0, -clampv * 3), (np.inf, 0.0, 0.0), (0.25, 0.25, 0.25), (0.0, -np.inf, 1.0)], f32)
            pixel = np.array([3, W * H, 3, 3, 3, 4, W * H + 1000, W * H - 1], np.uint32)
            sample = np.array([1, 2, 1, 11, 10, 0, 3, 15], np.uint32)
            states = F.states_for(pixel, special, seed=p.seed)
            states["sample"] = sample
            status = stage(pb, states, kw)
            acc.deposit(pb)
            want, counters = R.deposit(states, status, W, H, SPP, K)
            state, clean = sums_between_canaries(acc)
            assert clean and np.array_equal(state, want) and R.counters_of(acc.info()) == counters
            assert counters == dict(deposited=3, dropped=3, clamped=1, skipped=2)
            flat = state.reshape(W * H, K, 4)
            assert flat[3, 1].tolist() == [int(f32(31.999) * f32(2 ** 26)), -int(f32(31.999) * f32(2 ** 26)), 1 << 26, 2]     # NaN: count only
            assert flat[3, 2].tolist() == [int(f32(clampv) * f32(2 ** 26)), 1 << 26, -int(f32(clampv) * f32(2 ** 26)), 1]
            assert flat[4, 0].tolist() == [0, 0, 0, 1] and flat[W * H - 1, 7].tolist() == [0, 0, 0, 1]
            assert int((flat[:, :, 3]).sum()) == 6 and not flat[W * H - 1, :7].any()
            rgb, se = acc.resolve(want_stderr=True)
            ref, ref_se = R.resolve(state, R.GINI)
            assert np.array_equal(bits(rgb), bits(ref)) and np.array_equal(bits(se), bits(ref_se))

            # batch lengths on both sides of a wave and of a workgroup, every pixel pattern, the special radiances
            seen = dict.fromkeys(R.COUNTERS, 0)
            for n in LENGTHS:
                for pname, pixel in F.pixel_patterns(n, W * H).items():
                    states = F.states_for(pixel, F.radiances(n, SPP, seed=len(pname)), seed=p.seed)
                    states["sample"] = (np.arange(n) * 7 + n) % 40
                    acc.reset()
                    status = stage(pb, states, kw)
                    acc.deposit(pb)
                    want, counters = R.deposit(states, status, W, H, SPP, K)
                    assert np.array_equal(acc.debug_sums(), want), (n, pname)
                    assert R.counters_of(acc.info()) == counters and acc.info().deposits == 1, (n, pname)
                    for k in seen:
                        seen[k] += counters[k]
            assert all(seen.values()), seen
    finally:
        ds.close()


# ---------------------------------------------------------------- 4. flags, orders, reset, refusals
def test_six_orders_reset_and_resolve_arguments(device, host_scenes):
    lib = device
    hs, cam = host_scenes("cornell_box")
    W, H, spp = 24, 16, 3
    q = hs.params(W, spp, 8, seed=7, height=H)
    ds = DeviceScene(hs.desc)
    try:
        with ds.film(cam, q) as film, ds.splat(W, H, spp, filter=ffi.VK_SPLAT_TENT, radius=1.0) as sp, ds.robust(W, H, spp, buckets=2) as acc, \
                ds.paths(W * H * spp) as pb:
            takers = {"film": lambda: film.deposit(pb), "splat": lambda: sp.deposit(pb), "robust": lambda: acc.deposit(pb)}
            first = None
            for order in itertools.permutations(takers):
                film.reset()
                sp.reset()
                acc.reset()
                film.emit(pb, 0, 0, W, H, 0, spp)
                assert pb.step(100000).live == 0
                for who in order:
                    takers[who]()
                got = (film.debug_sums().tobytes(), sp.debug_sums().tobytes(), acc.debug_sums().tobytes(),
                       bytes(film.info()), bytes(sp.info()), bytes(acc.info()))
                first = first or got
                assert got == first, order
                # each has taken the batch: a second deposit of any is refused
                assert lib.vk_robust_deposit(acc._h, pb._h) == ffi.VK_ERR_BAD_ARG
                assert b"deposited into a robust accumulator since its last begin or emit" in lib.vk_last_error()
                assert lib.vk_film_deposit(film._h, pb._h) == ffi.VK_ERR_BAD_ARG and lib.vk_splat_deposit(sp._h, pb._h, None) == ffi.VK_ERR_BAD_ARG
                assert acc.debug_sums().tobytes() == first[2] and bytes(acc.info()) == first[5]
            states, status = pb.results()
            want, counters = R.deposit(states, status, W, H, spp, 2)
            assert np.array_equal(acc.debug_sums(), want) and R.counters_of(acc.info()) == counters
            assert np.array_equal(bits(acc.resolve(mode=R.MEAN)), bits(film.resolve(spp)))
            # vk_paths_begin clears the flag as vk_film_emit does
            stage(pb, states[:100], S.shade_kwargs(q, q.integrator, 8))
            acc.deposit(pb)
            assert acc.info().deposits == 2
            # how: other buckets, an unknown mode, a non-zero _pad are refused and write nothing; 0 buckets and the accumulator's own pass
            img, se = np.full((H, W, 3), 7, f32), np.full((H, W, 3), 7, f32)
            for fields, word in (((8, 0, 0, 0), b"how->buckets must be 0 or the accumulator's"), ((2, 3, 0, 0), b"unknown mode"),
                                 ((0, 2, 0, 5), b"_pad must be 0")):
                how = ffi.RobustParams(*fields)
                assert lib.vk_robust_resolve(acc._h, C.byref(how), img.ctypes.data, se.ctypes.data) == ffi.VK_ERR_BAD_ARG, fields
                assert word in lib.vk_last_error() and (img == 7).all() and (se == 7).all()
            for buckets in (0, 2):
                how = ffi.RobustParams(buckets, ffi.VK_ROBUST_MEAN, 99, 0)
                assert lib.vk_robust_resolve(acc._h, C.byref(how), img.ctypes.data, None) == ffi.VK_OK
                assert np.array_equal(bits(img), bits(acc.resolve(mode=R.MEAN))) and (se == 7).all()
            # reset zeroes sums and counters, and the accumulator takes the same frame again
            acc.reset()
            assert not acc.debug_sums().any() and bytes(acc.info())[16:] == bytes(48)
            rgb, se = acc.resolve(want_stderr=True)
            assert not rgb.any() and not se.any()
            film.emit(pb, 0, 0, W, H, 0, spp)
            assert pb.step(100000).live == 0
            acc.deposit(pb)
            assert np.array_equal(acc.debug_sums(), want) and acc.info().deposits == 1
            lib.vk_robust_destroy(None)
    finally:
        ds.close()


def test_refusals_leave_accumulator_and_batch_as_they_were(device, host_scenes):
    lib = device
    hs, cam = host_scenes("cornell_box")
    W, H = 24, 16
    q = hs.params(W, 1, 8, seed=9, height=H)
    ds, other = DeviceScene(hs.desc), DeviceScene(hs.desc)
    try:
        h = C.c_void_p(0x77)
        for fields, word in (((1, 0, 0, 0), b"buckets must be in 2..16"), ((17, 0, 0, 0), b"buckets must be in 2..16"),
                             ((8, 7, 0, 0), b"unknown mode"), ((8, 1, 2, 1), b"_pad must be 0")):
            bad = ffi.RobustParams(*fields)
            assert lib.vk_robust_create(ds._h, W, H, 1, C.byref(bad), C.byref(h)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error()
        ok = ffi.RobustParams(8, ffi.VK_ROBUST_GINI, 0, 0)
        assert lib.vk_robust_create(ds._h, 8192, 8192, 1, C.byref(ok), C.byref(h)) == ffi.VK_ERR_BAD_ARG and b"exceeds 2^27" in lib.vk_last_error()
        assert lib.vk_robust_create(ds._h, W, H, 1, None, C.byref(h)) == ffi.VK_ERR_BAD_ARG and h.value == 0x77
        # trim is TRIM's alone
        with ds.robust(W, H, 1, buckets=4, mode=ffi.VK_ROBUST_GINI, trim=0xFFFFFFFF) as g:
            assert g.info().buckets == 4
        with ds.film(cam, q) as film, ds.robust(W, H, 1, buckets=4) as acc, ds.paths(W * H) as pb, other.paths(W * H) as foreign, \
                ds.paths(16) as never, ds.paths(100) as run:
            film.emit(pb, 0, 0, W, H, 0, 1)
            pb.step(100000)
            acc.deposit(pb)
            sums0 = acc.debug_sums().tobytes()

            def refused(batch, word):
                before, ai = bytes(batch.info()), bytes(acc.info())
                assert lib.vk_robust_deposit(acc._h, batch._h) == ffi.VK_ERR_BAD_ARG, word
                assert word in lib.vk_last_error(), lib.vk_last_error()
                assert bytes(batch.info()) == before and bytes(acc.info()) == ai and acc.debug_sums().tobytes() == sums0, word

            refused(pb, b"deposited into a robust accumulator since its last begin or emit")
            refused(foreign, b"belongs to another scene")
            refused(never, b"before vk_paths_begin or vk_film_emit")
            film.emit(pb, 0, 0, W, H, 0, 1)
            pb.step(1)
            assert pb.info().live > 0
            refused(pb, b"live paths (step or cull them first)")
            film.regen_begin(run, 0, 0, W, H, 0, 1)
            refused(run, b"regenerating path batch")
            assert lib.vk_robust_deposit(None, pb._h) == ffi.VK_ERR_BAD_ARG and lib.vk_robust_deposit(acc._h, None) == ffi.VK_ERR_BAD_ARG
            img = np.full(W * H * 3, 7, f32)
            assert lib.vk_robust_resolve(None, None, img.ctypes.data, None) == ffi.VK_ERR_BAD_ARG
            assert lib.vk_robust_resolve(acc._h, None, None, img.ctypes.data) == ffi.VK_ERR_BAD_ARG
            assert lib.vk_robust_reset(None) == ffi.VK_ERR_BAD_ARG and (img == 7).all()
            assert acc.debug_sums().tobytes() == sums0
            # the live batch is as it was: it finishes and goes in
            pb.step(100000)
            acc.deposit(pb)
            assert acc.info().deposits == 2 and np.array_equal(acc.debug_sums(), 2 * np.frombuffer(sums0, np.int64).reshape(H, W, 4, 4))
            lib.vk_robust_destroy(None)
    finally:
        other.close()
        ds.close()
