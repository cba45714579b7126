"""Reconstruction filters on the device.  THE ANCHOR: a film's camera paths deposited into a BOX accumulator of radius 0.5 give
vk_render's frame bit for bit, with the film's counters.  The deposit alone on hand-made finished batches — every filter setting, every
pixel pattern, batch lengths on both sides of a wave and of a workgroup, frames narrower than the footprint — against tests/splat_ref.py
in both kernel forms, whose bytes are equal; row wraps and a random pixel order inside a workgroup.  The sums of a real frame do not
depend on how it was cut into batches or in what order.  The caller's own positions.  Flags, side effects and refusals."""
import ctypes as C

import numpy as np
import pytest

import film_ref as F
import shade_ref as S
import splat_ref as R
from vecchio_amd import DeviceScene, ffi
from vecchio_amd.scene import RAY_DTYPE, make_path_states

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMS = (ffi.VK_DEBUG_SPLAT_FORM_PLAIN, ffi.VK_DEBUG_SPLAT_FORM_TILED)
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1000)         # wave and workgroup boundaries
MITCHELL2 = R.FILTERS[4]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def splat_of(ds, W, H, spp, sp):
    return ds.splat(W, H, spp, filter=sp[0], radius=sp[1], b=sp[2], c=sp[3])


def dead_rays(n):
    rays = np.zeros(n, RAY_DTYPE)
    rays["direction"][:, 2], rays["tmax"] = -1.0, np.inf
    return rays


def stage(pb, states, kw):
    """a finished batch whose results are exactly `states`, every status VK_PATHS_CULLED: begun and retired at once (the way
    tests/test_gpu_film.py stages its deposit batches)"""
    n = len(states)
    pb.begin(dead_rays(n), states, **kw)
    pb.cull(np.zeros(n, np.uint8))
    return np.full(n, ffi.VK_PATHS_CULLED, np.uint32)


def in_both_forms(acc, pb, states, kw, want, counters, what, positions=None):
    got = []
    for form in FORMS:
        acc.reset()
        acc.debug_form(form)
        stage(pb, states, kw)
        acc.deposit(pb, positions)
        sums = acc.debug_sums()
        assert np.array_equal(sums, want), (what, form)
        inf = acc.info()
        assert R.counters_of(inf) == counters and inf.deposits == 1, (what, form, R.counters_of(inf), counters)
        got.append(sums.tobytes())
    assert got[0] == got[1], what


# ---------------------------------------------------------------- 1. THE ANCHOR
def anchor_windows(W, H, spp):
    """tests/test_gpu_film.py's windows — a partition of 40 x 13 x 3 samples into every awkward shape — cut to this frame's W columns,
    with the samples beyond its three in one window more"""
    import test_gpu_film as G
    assert H == G.FH and W <= G.FW and spp > G.SPP
    out = [(x0, y0, min(w, W - x0), h, s0, ns) for x0, y0, w, h, s0, ns in G.WINDOWS if x0 < W]
    return out + [(0, 0, W, H, G.SPP, spp - G.SPP)]


@pytest.mark.parametrize("name", ["random_spheres_iow", "cornell_box"])
def test_box_of_radius_half_is_vk_render(name, device, host_scenes):
    hs, cam = host_scenes(name)
    W, H, spp = 21, 13, 4
    q = hs.params(W, spp, 50, seed=5, height=H)
    windows = anchor_windows(W, H, spp)
    seen = np.zeros(W * H * spp, int)
    for w in windows:
        seen[F.dump_index(W, spp, *w)] += 1
    assert (seen == 1).all()
    ds = DeviceScene(hs.desc)
    try:
        frame, _ = ds.render(cam, q)
        with ds.film(cam, q) as film, splat_of(ds, W, H, spp, R.FILTERS[0]) as acc, ds.paths(300) as a, ds.paths(273) as b:
            for k, j in enumerate(np.random.default_rng(3).permutation(len(windows))):
                pb = (a, b)[k % 2]
                film.emit(pb, *windows[j])
                assert pb.step(100000).live == 0
                if k % 2:
                    film.deposit(pb)
                    acc.deposit(pb)
                else:
                    acc.deposit(pb)
                    film.deposit(pb)
            img = acc.resolve()
            assert np.array_equal(bits(img), bits(film.resolve(spp))) and np.array_equal(bits(img), bits(frame))
            sums = acc.debug_sums()
            assert np.array_equal(sums[..., :3], film.debug_sums()) and (sums[..., 3] == spp << 26).all()
            fi, si = film.info(), acc.info()
            assert (si.deposited, si.dropped, si.clamped, si.skipped) == (fi.deposited, fi.dropped, fi.clamped, fi.skipped)
            assert si.deposited == W * H * spp == si.contributions and si.deposits == len(windows)
            assert (si.width, si.height, si.samples_per_pixel, si.filter) == (W, H, spp, ffi.VK_SPLAT_BOX)
            ms = acc.last_ms()
            assert ms[0] > 0 and ms[1] > 0
    finally:
        ds.close()


# ---------------------------------------------------------------- 2. exact sums, both forms
@pytest.mark.parametrize("frame", R.FRAMES, ids=[f"{w}x{h}" for w, h in R.FRAMES])
@pytest.mark.parametrize("sp", R.FILTERS, ids=R.FILTER_IDS)
def test_deposit_alone_in_both_forms(sp, frame, device, host_scenes):
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    W, H = frame
    spp = 40                                                  # the clamp is 1.3e11 / (40 F), below 1e10
    budget = spp * R.side(sp[1]) ** 2
    kw = S.shade_kwargs(p, p.integrator, 8)
    seen = dict.fromkeys(R.COUNTERS, 0)
    ds = DeviceScene(desc)
    try:
        with ds.paths(max(LENGTHS)) as pb, splat_of(ds, W, H, spp, sp) as acc:
            for n in LENGTHS:
                for name, pixel in F.pixel_patterns(n, W * H).items():
                    states = R.states_with_samples(pixel, F.radiances(n, budget, seed=len(name)), seed=p.seed)
                    want, counters = R.deposit(states, np.full(n, ffi.VK_PATHS_CULLED, np.uint32), W, H, spp, sp)
                    in_both_forms(acc, pb, states, kw, want, counters, f"{sp} {W}x{H} n {n} {name}")
                    for k in seen:
                        seen[k] += counters[k]
        assert all(seen.values()), seen
    finally:
        ds.close()


@pytest.mark.parametrize("sp", [R.FILTERS[3], MITCHELL2], ids=["tent1.5", "mitchell"])
def test_row_wraps_and_a_random_pixel_order_inside_a_workgroup(sp, device, host_scenes):
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    W, H, spp = 64, 5, 2
    kw = S.shade_kwargs(p, p.integrator, 8)
    ds = DeviceScene(desc)
    try:
        with ds.paths(W * H * spp) as pb, splat_of(ds, W, H, spp, sp) as acc:
            # a 37-wide window: 256 consecutive ids cross three of its row ends
            pixel, sample = F.ids_of(W, 10, 0, 37, H, 0, spp)
            # every pixel twice, in random order: next to no target lies in a workgroup's tile
            perm = np.random.default_rng(4).permutation(np.repeat(np.arange(W * H, dtype=np.uint32), spp))
            for what, px, smp in (("window", pixel, sample), ("permutation", perm, np.arange(len(perm)) % spp)):
                states = F.states_for(px, F.radiances(len(px), spp * 16, seed=8), seed=p.seed)
                states["sample"] = smp
                want, counters = R.deposit(states, np.full(len(px), ffi.VK_PATHS_CULLED, np.uint32), W, H, spp, sp)
                in_both_forms(acc, pb, states, kw, want, counters, (sp, what))
    finally:
        ds.close()


# ---------------------------------------------------------------- 3. partition independence
def test_any_partition_and_any_order_give_the_same_sums(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    W, H, spp = 21, 13, 3
    q = hs.params(W, spp, 12, seed=6, height=H)
    n = W * H * spp
    ds = DeviceScene(hs.desc)
    try:
        with ds.film(cam, q) as film, splat_of(ds, W, H, spp, MITCHELL2) as acc:
            with ds.paths(n + 5) as big:
                img = acc.render(film, big)
                assert acc.info().deposits == 1
                states, status = big.results()
            want, counters = R.deposit(states, status, W, H, spp, MITCHELL2)
            first = acc.debug_sums()
            assert np.array_equal(first, want) and R.counters_of(acc.info()) == counters
            assert counters["deposited"] + counters["dropped"] == n and counters["skipped"] == 0
            assert np.array_equal(bits(img), bits(R.resolve(want)))
            for cap in (spp, 64, 65):
                with ds.paths(cap) as pb:
                    for order in (0, 1):
                        acc.reset()
                        windows = list(film.windows(cap))
                        if order:
                            windows = [windows[j] for j in np.random.default_rng(cap).permutation(len(windows))]
                        fed = np.zeros((H, W, 4), np.int64)
                        for win in windows:
                            film.emit(pb, *win)
                            assert pb.step(100000).live == 0
                            acc.deposit(pb)
                            if cap == 65:                     # the reference fed with these very batches, window by window
                                fed, _ = R.deposit(*pb.results(), W, H, spp, MITCHELL2, sums=fed)
                        assert acc.debug_sums().tobytes() == first.tobytes(), (cap, order)
                        assert R.counters_of(acc.info()) == counters and acc.info().deposits == len(windows) > 1
                        if cap == 65:
                            assert np.array_equal(fed, want)
            assert np.array_equal(bits(acc.resolve()), bits(img))
    finally:
        ds.close()


# ---------------------------------------------------------------- 4. the caller's own positions
@pytest.mark.parametrize("sp", [R.FILTERS[0], R.FILTERS[2], MITCHELL2], ids=["box0.5", "tent1", "mitchell"])
def test_positions_of_the_callers_own(sp, device, host_scenes):
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    W, H, spp = 21, 13, 2
    pos = R.boundary_positions(W, H)
    n = len(pos)
    rays = S.rays_of(cam)[:n]
    assert len(rays) == n
    kw = S.shade_kwargs(p, p.integrator, 8)
    ds = DeviceScene(desc)
    try:
        with ds.paths(n) as pb, splat_of(ds, W, H, spp, sp) as acc:
            states = make_path_states(n, seed=21)
            states["pixel"] = W * H + 3                       # not read with positions
            pb.begin(rays, states, **kw)
            assert pb.step(100000).live == 0
            res, status = pb.results()
            want, counters = R.deposit(res, status, W, H, spp, sp, pos)
            assert counters["deposited"] > 20 and counters["skipped"] >= 9
            got = []
            for form in FORMS:
                acc.reset()
                acc.debug_form(form)
                if form != FORMS[0]:
                    pb.begin(rays, states, **kw)
                    pb.step(100000)
                acc.deposit(pb, pos)
                assert np.array_equal(acc.debug_sums(), want) and R.counters_of(acc.info()) == counters, (sp, form)
                got.append(acc.debug_sums().tobytes())
            assert got[0] == got[1]
            # without positions the same batch is skipped whole: its pixels lie outside the frame
            acc.reset()
            pb.begin(rays, states, **kw)
            pb.step(100000)
            acc.deposit(pb)
            assert not acc.debug_sums().any() and acc.info().skipped == n
            # the hand-made batch again, positions on every boundary, through the staged route
            hand = R.states_with_samples(np.zeros(n, np.uint32), F.radiances(n, spp * 16, seed=5), seed=p.seed)
            want, counters = R.deposit(hand, np.full(n, ffi.VK_PATHS_CULLED, np.uint32), W, H, spp, sp, pos)
            in_both_forms(acc, pb, hand, kw, want, counters, (sp, "hand"), positions=pos)
    finally:
        ds.close()


# ---------------------------------------------------------------- 5. flags and side effects
def test_flags_reset_and_two_accumulators(device, host_scenes):
    lib = device
    hs, cam = host_scenes("cornell_box")
    W, H, spp = 21, 13, 2
    q = hs.params(W, spp, 8, seed=7, height=H)
    ds = DeviceScene(hs.desc)
    try:
        with ds.film(cam, q) as film, splat_of(ds, W, H, spp, MITCHELL2) as a, splat_of(ds, W, H, spp, R.FILTERS[2]) as b, \
                ds.paths(W * H * spp) as pb:
            def whole():
                film.emit(pb, 0, 0, W, H, 0, spp)
                assert pb.step(100000).live == 0

            whole()
            a.deposit(pb)
            sums_a, info_a = a.debug_sums(), bytes(a.info())
            # a second deposit without a new begin: refused, nothing written; the film and the other accumulator still take the batch
            assert lib.vk_splat_deposit(a._h, pb._h, None) == ffi.VK_ERR_BAD_ARG
            assert b"deposited into an accumulator since its last begin or emit" in lib.vk_last_error()
            assert lib.vk_splat_deposit(b._h, pb._h, None) == ffi.VK_ERR_BAD_ARG
            assert a.debug_sums().tobytes() == sums_a.tobytes() and bytes(a.info()) == info_a and not b.debug_sums().any()
            film.deposit(pb)
            film_sums = film.debug_sums()
            # the other order: the film first
            whole()
            film.reset()
            film.deposit(pb)
            b.deposit(pb)
            assert np.array_equal(film.debug_sums(), film_sums)
            states, status = pb.results()
            want_a, ca = R.deposit(states, status, W, H, spp, MITCHELL2)
            want_b, cb = R.deposit(states, status, W, H, spp, R.FILTERS[2])
            assert np.array_equal(sums_a, want_a) and np.array_equal(b.debug_sums(), want_b)
            assert R.counters_of(a.info()) == ca and R.counters_of(b.info()) == cb
            # two accumulators, alternately: neither disturbs the other
            whole()
            b.deposit(pb)
            assert np.array_equal(b.debug_sums(), 2 * want_b) and a.debug_sums().tobytes() == sums_a.tobytes()
            # reset zeroes sums and counters, and the accumulator takes the same frame again
            a.reset()
            assert not a.debug_sums().any() and bytes(a.info())[16:] == bytes(48) and not a.resolve().any()
            whole()
            a.deposit(pb)
            assert np.array_equal(a.debug_sums(), want_a) and a.info().deposits == 1
            lib.vk_splat_destroy(None)
    finally:
        ds.close()


def test_an_accumulator_leaves_the_render_the_log_and_a_progress_handle_alone(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    p = hs.params(96, 4, 20, seed=3)
    fq = hs.params(24, 3, 20, seed=4, height=16)
    ds = DeviceScene(hs.desc)
    try:
        before, _ = ds.render(cam, p)
        ms, requeued = ds.last_kernel_ms(), ds.last_requeued_samples()
        launches = [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)]
        with ds.film(cam, fq) as film, splat_of(ds, 24, 16, 3, MITCHELL2) as acc, ds.paths(24 * 16 * 3) as pb:
            acc.render(film, pb)
            first = acc.debug_sums().copy()
            assert abs(ds.last_kernel_ms() - ms) < 1e-4 and ds.last_requeued_samples() == requeued
            assert [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)] == launches and launches
            after, _ = ds.render(cam, p)
            np.testing.assert_array_equal(bits(before), bits(after))
            acc.reset()
            acc.render(film, pb)
            np.testing.assert_array_equal(acc.debug_sums(), first)
            # a progress handle interrupted by a filtered frame is one that was not
            with ds.progress(cam, p) as pr:
                pr.step(2)
                moments = pr.moments()[0].copy()
                info = bytes(pr.info())
                acc.reset()
                acc.render(film, pb)
                assert bytes(pr.info()) == info
                np.testing.assert_array_equal(pr.moments()[0], moments)
                interrupted, _ = pr.step(2)
            with ds.progress(cam, p) as pr:
                pr.step(2)
                plain, _ = pr.step(2)
            np.testing.assert_array_equal(bits(interrupted), bits(plain))
    finally:
        ds.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_accumulator_and_batch_as_they_were(device, host_scenes):
    lib = device
    hs, cam = host_scenes("cornell_box")
    W, H = 21, 13
    q = hs.params(W, 1, 8, seed=9, height=H)
    ds, other = DeviceScene(hs.desc), DeviceScene(hs.desc)
    try:
        h = C.c_void_p(0x77)
        for fields, word in (((7, 1.0, 0.0, 0.0), b"unknown filter"), ((1, 0.25, 0.0, 0.0), b"radius must be finite and in [0.5, 2]"),
                             ((1, float("nan"), 0.0, 0.0), b"radius must be finite"), ((2, 2.0, 1.5, 0.0), b"b and c must be finite"),
                             ((2, 2.0, 0.0, float("inf")), b"b and c must be finite")):
            bad = ffi.SplatParams(*fields)
            assert lib.vk_splat_create(ds._h, W, H, 1, C.byref(bad), C.byref(h)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error()
        ok = ffi.SplatParams(*MITCHELL2)
        assert lib.vk_splat_create(ds._h, 8200, 8200, 1, C.byref(ok), C.byref(h)) == ffi.VK_ERR_BAD_ARG
        assert lib.vk_splat_create(ds._h, W, H, 1, None, C.byref(h)) == ffi.VK_ERR_BAD_ARG and h.value == 0x77
        # b and c are MITCHELL's alone
        with ds.splat(W, H, 1, filter=ffi.VK_SPLAT_TENT, radius=1.0, b=float("nan"), c=9.0) as tent:
            assert tent.info().filter == ffi.VK_SPLAT_TENT
        with ds.film(cam, q) as film, splat_of(ds, W, H, 1, MITCHELL2) as acc, ds.paths(W * H) as pb, other.paths(W * H) as foreign, \
                ds.paths(16) as never, ds.paths(100) as run:
            film.emit(pb, 0, 0, W, H, 0, 1)
            pb.step(100000)
            acc.deposit(pb)
            sums0 = acc.debug_sums().tobytes()
            pos = np.zeros((W * H, 2), f32)

            def refused(batch, word, positions=None):
                before, ai = bytes(batch.info()), bytes(acc.info())
                ptr = positions.ctypes.data if positions is not None else None
                assert lib.vk_splat_deposit(acc._h, batch._h, ptr) == ffi.VK_ERR_BAD_ARG, word
                assert word in lib.vk_last_error(), lib.vk_last_error()
                assert bytes(batch.info()) == before and bytes(acc.info()) == ai and acc.debug_sums().tobytes() == sums0, word

            refused(pb, b"deposited into an accumulator since its last begin or emit")
            refused(pb, b"deposited into an accumulator since its last begin or emit", pos)
            refused(foreign, b"belongs to another scene")
            refused(never, b"before vk_paths_begin or vk_film_emit")
            film.emit(pb, 0, 0, W, H, 0, 1)
            pb.step(1)
            assert pb.info().live > 0
            refused(pb, b"live paths (step or cull them first)")
            film.regen_begin(run, 0, 0, W, H, 0, 1)
            refused(run, b"regenerating path batch")
            assert lib.vk_splat_deposit(None, pb._h, None) == ffi.VK_ERR_BAD_ARG and lib.vk_splat_deposit(acc._h, None, None) == ffi.VK_ERR_BAD_ARG
            img = np.full(W * H * 3, 7, f32)
            assert lib.vk_splat_resolve(None, img.ctypes.data) == ffi.VK_ERR_BAD_ARG and lib.vk_splat_resolve(acc._h, None) == ffi.VK_ERR_BAD_ARG
            assert lib.vk_splat_reset(None) == ffi.VK_ERR_BAD_ARG and (img == 7).all()
            assert lib.vk_debug_splat_form(acc._h, 3) == ffi.VK_ERR_BAD_ARG and b"unknown deposit form" in lib.vk_last_error()
            assert acc.debug_sums().tobytes() == sums0
            # the live batch is as it was: it finishes and goes in
            pb.step(100000)
            acc.deposit(pb)
            assert acc.info().deposits == 2 and np.array_equal(acc.debug_sums(), 2 * np.frombuffer(sums0, np.int64).reshape(H, W, 4))
    finally:
        other.close()
        ds.close()
