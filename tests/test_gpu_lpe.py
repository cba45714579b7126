"""Light-path layers on the device.  TAG PARITY: a film's camera paths stepped by vk_lpe_step in slices of 1, 3 and "to the end", window
by window — vk_lpe_tags is the tag tests/lpe_ref.py derives from every bounce of the CPU emulation, bit for bit, with the handle's
roulette rule too, and a twin batch stepped by vk_paths_step reads byte for byte the same.  LAYER PARITY: the raw state is the
restatement's, the layers add up to the film's sums, the counters are the film's, VK_LPE_ALL is vk_film_resolve's and vk_render's frame
and every layer's image and share are the restatement's, bit for bit.  The deposit alone on injected results and tags.  The 24 orders
of film, splat, robust and layer deposits, reset, vk_paths_cull between steps, refusals.  RADIOMETRY: the integrating sphere's frame
split by the segment the lamp was met on, against the closed form within d segments."""
import ctypes as C
import itertools

import numpy as np
import pytest

import emu_film_ffi
import emu_paths_ffi
import film_ref as F
import lpe_ref as L
import radiometry_ref as R
import robust_ref
import shade_ref as S
import test_gpu_robust as TR
from vecchio_amd import DeviceScene, ffi
from vecchio_amd.scene import STANDARD_LAYERS, lpe_events, lpe_rule, standard_rules

pytestmark = pytest.mark.gpu
f32 = np.float32
u32 = np.uint32
SPP = L.SPP
LENGTHS = TR.LENGTHS
bits = TR.bits
ENDED, MISS, CULLED = (ffi.VK_SHADE_ENDED,), (ffi.VK_SHADE_MISS,), (ffi.VK_PATHS_CULLED,)


# ---------------------------------------------------------------- 1. tag parity
CASES = [(k, n, i, fr, None) for k, n, i in L.SCENES for fr in L.FRAMES] + [L.SCENES[0] + (L.FRAMES[0], L.ROULETTE)]


@pytest.mark.parametrize("kind,name,integrator,frame,rule", CASES,
                         ids=[f"{c[1]}-{c[3][0]}x{c[3][1]}" + ("-roulette" if c[4] else "") for c in CASES])
def test_tag_parity_and_the_twin_batch(kind, name, integrator, frame, rule, device, host_scenes):
    desc, cam, p = L.scene(kind, name, host_scenes)
    W, H = frame
    q = L.frame_params(p, W, H, integrator)
    states_f, status_f, sig_f, term_f, taken_f = L.emulated_frame(desc, cam, q, name, rule)
    if rule:
        assert (status_f == ffi.VK_PATHS_CULLED).any()
    else:
        assert (taken_f > 7).any()                               # (tests/test_lpe_emu.py: nibble 7 is not nibble 6's copy)
    wins = TR.windows_of(W, H)
    ds = DeviceScene(desc)
    batches = {}
    try:
        for cap in sorted({cap for _, cap in wins}):
            batches[cap] = (ds.paths(cap), ds.paths(cap))
            for pb in batches[cap]:
                pb.set_roulette(*(rule or (None,)))
        recorded = 0
        with ds.film(cam, q) as film, ds.lpe(W, H, SPP, capacity=257) as lpe:
            for j in np.random.default_rng(W).permutation(len(wins)):
                win, cap = wins[j]
                pb, twin = batches[cap]
                idx = F.dump_index(W, SPP, *win)
                film.emit(pb, *win)
                film.emit(twin, *win)
                ids, rays, states = pb.read()
                er, es = emu_film_ffi.emit(cam, q, *win)
                assert np.array_equal(ids, np.arange(len(idx))) and rays.tobytes() == er.tobytes() and states.tobytes() == es.tobytes()
                # the twin, a bounce a call: what vk_paths_read gives after every bounce
                reads, infos = [], []
                while True:
                    infos.append(twin.step(1))
                    reads.append(tuple(a.tobytes() for a in twin.read()))
                    if infos[-1].live == 0:
                        break
                n_slice = (1, 3, 100000)[int(j) % 3]
                done = 0
                while True:
                    info = lpe.step(pb, n_slice)
                    assert info.bounces == min(n_slice, len(reads) - done) and info.kernel_launches == 6 * info.bounces, (win, done)
                    part = infos[done:done + info.bounces]
                    done += info.bounces
                    assert (info.traced, info.missed, info.ended, info.bad, info.live) == \
                        (sum(i.traced for i in part), sum(i.missed for i in part), sum(i.ended for i in part), sum(i.bad for i in part), part[-1].live)
                    assert tuple(a.tobytes() for a in pb.read()) == reads[done - 1], (name, win, done)
                    assert bytes(pb.info()) == bytes(twin.info()) if done == len(reads) else pb.info().bounces == done
                    recorded += info.traced
                    if info.live == 0:
                        break
                assert done == len(reads)
                a, b = pb.results(), twin.results()
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (name, win)
                assert np.array_equal(a[1], status_f[idx]), (name, win)
                sig, term = lpe.tags(pb)
                assert np.array_equal(sig, sig_f[idx]) and np.array_equal(term, term_f[idx]), (name, win, sig[:4], sig_f[idx][:4])
            assert lpe.info().recorded == recorded == int(taken_f.sum())
            assert lpe.last_ms()[0] > 0
    finally:
        for pair in batches.values():
            for pb in pair:
                pb.close()
        ds.close()


# ---------------------------------------------------------------- 2. layer parity
def light_materials(desc):
    d = desc.contents
    return [i for i in range(d.n_materials) if d.materials[i].kind == ffi.VK_MAT_DIFFUSE_LIGHT]


def depth_and_emitter_rules(desc):
    """(rules, n_layers, rest): light met within three bounces / later, by the first DiffuseLight material; the sky seen directly /
    after bounces; everything else in layer 4"""
    lights = light_materials(desc) or [0]
    return [lpe_rule(0, status=ENDED, depth=(2, 4), emitter=lights[0]), lpe_rule(1, status=ENDED, depth=(5, 0xFFFFFFFF), emitter=lights[0]),
            lpe_rule(2, status=MISS, depth=(1, 1)), lpe_rule(3, status=MISS)], 5, 4


@pytest.mark.parametrize("frame", L.FRAMES, ids=[f"{w}x{h}" for w, h in L.FRAMES])
@pytest.mark.parametrize("kind,name,integrator", L.SCENES, ids=[s[1] for s in L.SCENES])
def test_layer_parity(kind, name, integrator, frame, device, host_scenes):
    desc, cam, p = L.scene(kind, name, host_scenes)
    W, H = frame
    q = L.frame_params(p, W, H, integrator)
    _, status_f, sig_f, term_f, _ = L.emulated_frame(desc, cam, q, name)
    wins = TR.windows_of(W, H)
    sets = [(standard_rules(), len(STANDARD_LAYERS), STANDARD_LAYERS.index("rest")), depth_and_emitter_rules(desc)]
    ds = DeviceScene(desc)
    try:
        render, _ = ds.render(cam, q)
        accs = [ds.lpe(W, H, SPP, 257, rules, n, rest) for rules, n, rest in sets]
        batches = {cap: ds.paths(cap) for cap in sorted({cap for _, cap in wins})}
        want = [np.zeros((H, W, n, 4), np.int64) for _, n, _ in sets]
        counters = dict.fromkeys(L.COUNTERS, 0)
        try:
            with ds.film(cam, q) as film:
                for j in np.random.default_rng(H).permutation(len(wins)):
                    win, cap = wins[j]
                    pb = batches[cap]
                    idx = F.dump_index(W, SPP, *win)
                    # (a batch goes into ONE layer accumulator per emit: the window is emitted again for each, and gives the same results)
                    for i, acc in enumerate(accs):
                        film.emit(pb, *win)
                        assert acc.step(pb, 100000).live == 0
                        if i == 0:
                            film.deposit(pb)
                            states, status = pb.results()
                        acc.deposit(pb)
                    for i, (rules, n, rest) in enumerate(sets):
                        want[i], c = L.deposit(states, status, sig_f[idx], term_f[idx], rules, n, rest, W, H, SPP, want[i])
                    for k in counters:
                        counters[k] += c[k]
                film_sums, fi = film.debug_sums(), film.info()
                film_img = film.resolve(SPP)
                assert np.array_equal(bits(film_img), bits(render))
                for (rules, n, rest), acc, w in zip(sets, accs, want):
                    what = f"{name} {W}x{H} layers {n}"
                    state = acc.debug_sums()
                    assert state.shape == (H, W, n, 4) and np.array_equal(state, w), what
                    assert np.array_equal(state[..., :3].sum(axis=2), film_sums), what
                    assert (state[..., 3].sum(axis=2) == SPP).all(), what
                    ai = acc.info()
                    assert L.counters_of(ai) == F.counters_of(fi) == counters, what
                    assert (ai.width, ai.height, ai.samples_per_pixel, ai.n_layers, ai.rest_layer, ai.n_rules, ai.capacity, ai.deposits) == \
                        (W, H, SPP, n, rest, len(rules), 257, len(wins)), what
                    both = acc.resolve(ffi.VK_LPE_ALL)
                    assert np.array_equal(bits(both), bits(film_img)) and np.array_equal(bits(both), bits(render)), what
                    assert np.array_equal(bits(both), bits(L.resolve(state, L.ALL, SPP)[0]))
                    used = 0
                    for layer in range(n):
                        rgb, share = acc.resolve(layer, want_share=True)
                        ref_rgb, ref_share = L.resolve(state, layer, SPP)
                        assert np.array_equal(bits(rgb), bits(ref_rgb)) and np.array_equal(bits(share), bits(ref_share)), (what, layer)
                        assert np.array_equal(bits(acc.resolve(layer)), bits(rgb))
                        used += bool(share.any())
                    assert used >= 3, (what, used)
                    assert np.array_equal(bits(acc.resolve(0, n=5)), bits(L.resolve(state, 0, 5)[0]))
                    assert np.array_equal(acc.debug_sums(), state), what          # the sums stay
                    ms = acc.last_ms()
                    assert ms[0] > 0 and ms[1] > 0 and ms[2] > 0
                if name == "cornell_box":
                    # the standard layers say what they are called: no medium in the box, the lamp seen directly, and the rest carries nothing
                    state = accs[0].debug_sums()
                    lay = {k: state[:, :, i] for i, k in enumerate(STANDARD_LAYERS)}
                    assert not lay["volume"].any() and not lay["rest"][..., :3].any() and lay["rest"][..., 3].any()
                    assert lay["emission"][..., :3].any() and lay["direct_diffuse"][..., :3].any() and lay["indirect"][..., :3].any()
        finally:
            for acc in accs:
                acc.close()
            for pb in batches.values():
                pb.close()
    finally:
        ds.close()


# ---------------------------------------------------------------- 3. the deposit alone, on injected results and tags
def sums_between_canaries(acc):
    """vk_debug_lpe_sums into the middle of a larger array: (the state, whether the rows around it are untouched)"""
    H, W, n = acc.height, acc.width, acc.n_layers
    buf = np.full((H + 4, W, n, 4), 0x5A5A5A5A5A5A5A5A, np.int64)
    assert acc._lib.vk_debug_lpe_sums(acc._h, buf[2:].ctypes.data) == ffi.VK_OK
    return buf[2:H + 2].copy(), bool((buf[:2] == 0x5A5A5A5A5A5A5A5A).all() and (buf[H + 2:] == 0x5A5A5A5A5A5A5A5A).all())


def inject(acc, pb, states, sig, term, kw):
    status = TR.stage(pb, states, kw)
    acc.debug_set_tags(pb, sig, term)
    got = acc.tags(pb)
    assert np.array_equal(got[0], sig) and np.array_equal(got[1], term)
    acc.deposit(pb)
    return status


def test_injected_results_and_tags(device, host_scenes):
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    W, H = 24, 16
    kw = S.shade_kwargs(p, p.integrator, 8)
    clampv = float(robust_ref.E.accum_clamp_for(SPP))
    rules = [lpe_rule(1, *lpe_events(2)),                                  # first match wins: the next rule asks the same
             lpe_rule(2, *lpe_events(2)),
             lpe_rule(3, status=ENDED + MISS),                             # the status mask: these results are all CULLED
             lpe_rule(4, depth=(3, 5)),                                    # both ends of the depth range
             lpe_rule(5, emitter=7),                                       # an emitter filter
             lpe_rule(0, 0xF0000000, 0x50000000, status=CULLED)]           # the last bounce's code
    ds = DeviceScene(desc)
    try:
        with ds.paths(max(LENGTHS)) as pb, ds.lpe(W, H, SPP, max(LENGTHS), rules, 7, 6) as acc, ds.lpe(W, H, SPP, max(LENGTHS), [], 3, 2) as bare:
            # one result per case, each in a pixel of its own
            sig = np.array([0x22222222, 0x00000003, 0x00000003, 0x00000003, 0x00000003, 0x00000003, 0x00000003, 0x50000003, 0x60000003], u32)
            depth = np.array([1, 2, 3, 5, 6, 9, 9, 9, 9], u32)
            term = np.array([7, 0, 0, 0, 0, 7, 8, 8, 0xFFFFFFFF], u32)
            layer = [1, 6, 4, 4, 6, 5, 6, 0, 6]
            n = len(sig)
            states = F.states_for(np.arange(n, dtype=u32), np.full((n, 3), 0.5, f32), seed=p.seed)
            states["depth"] = depth
            status = inject(acc, pb, states, sig, term, kw)
            assert L.layers_of(rules, 6, status, depth, sig, term).tolist() == layer
            state, clean = sums_between_canaries(acc)
            want, counters = L.deposit(states, status, sig, term, rules, 7, 6, W, H, SPP)
            assert clean and np.array_equal(state, want) and L.counters_of(acc.info()) == counters
            flat = state.reshape(W * H, 7, 4)
            for i, l in enumerate(layer):
                assert flat[i, l].tolist() == [1 << 25] * 3 + [1] and int(flat[i].any(axis=1).sum()) == 1, i
            assert not flat[n:].any() and not state[..., 2, :].any() and not state[..., 3, :].any()
            # no rule at all: everything in rest_layer
            status = inject(bare, pb, states, sig, term, kw)
            state, clean = sums_between_canaries(bare)
            assert clean and np.array_equal(state, L.deposit(states, status, sig, term, [], 3, 2, W, H, SPP)[0])
            assert not state[..., :2, :].any() and state[..., 2, 3].sum() == n and bare.info().n_rules == 0

            # a NaN (dropped, counted in its cell), a pixel at width * height (skipped: nothing touched), components at and beyond 31.999
            # and beyond the clamp (clamped), infinities
            acc.reset()
            special = np.array([(np.nan, 0.5, 0.5), (0.5, 0.5, 0.5), (31.999, -31.999, 1.0), (float(np.nextafter(f32(31.999), f32(40))), 1, 2),
                                (clampv * 2, 1.0, -clampv * 3), (np.inf, 0.0, 0.0), (0.25, 0.25, 0.25), (0.0, -np.inf, 1.0)], f32)
            pixel = np.array([3, W * H, 3, 3, 3, 4, W * H + 1000, W * H - 1], u32)
            sig = np.array([2, 2, 2, 3, 0x50000003, 2, 2, 3], u32)
            term = np.zeros(8, u32)
            states = F.states_for(pixel, special, seed=p.seed)
            status = inject(acc, pb, states, sig, term, kw)
            want, counters = L.deposit(states, status, sig, term, rules, 7, 6, W, H, SPP)
            state, clean = sums_between_canaries(acc)
            assert clean and np.array_equal(state, want) and L.counters_of(acc.info()) == counters
            assert counters == dict(deposited=3, dropped=3, clamped=1, skipped=2)
            flat = state.reshape(W * H, 7, 4)
            assert flat[3, 1].tolist() == [int(f32(31.999) * f32(2 ** 26)), -int(f32(31.999) * f32(2 ** 26)), 1 << 26, 2]     # NaN: count only
            assert flat[3, 0].tolist() == [int(f32(clampv) * f32(2 ** 26)), 1 << 26, -int(f32(clampv) * f32(2 ** 26)), 1]
            assert flat[4, 1].tolist() == [0, 0, 0, 1] and flat[W * H - 1, 6].tolist() == [0, 0, 0, 1]
            assert int(flat[:, :, 3].sum()) == 6
            for l in range(7):
                rgb, share = acc.resolve(l, want_share=True)
                ref = L.resolve(state, l, SPP)
                assert np.array_equal(bits(rgb), bits(ref[0])) and np.array_equal(bits(share), bits(ref[1]))

            # batch lengths on both sides of a wave and of a workgroup, every pixel pattern, the special radiances, random tags
            seen = dict.fromkeys(L.COUNTERS, 0)
            layers_seen = set()
            rng = np.random.default_rng(7)
            for n in LENGTHS:
                for pname, pixel in F.pixel_patterns(n, W * H).items():
                    states = F.states_for(pixel, F.radiances(n, SPP, seed=len(pname)), seed=p.seed)
                    states["depth"] = rng.integers(1, 8, n)
                    sig = (rng.choice([2, 3, 4], n) | (rng.choice([5, 1, 2], n) << 28)).astype(u32)
                    term = rng.choice([0, 7, 8, 0xFFFFFFFF], n).astype(u32)
                    acc.reset()
                    status = inject(acc, pb, states, sig, term, kw)
                    want, counters = L.deposit(states, status, sig, term, rules, 7, 6, W, H, SPP)
                    state, clean = sums_between_canaries(acc)
                    assert clean and np.array_equal(state, want), (n, pname)
                    assert L.counters_of(acc.info()) == counters and acc.info().deposits == 1, (n, pname)
                    layers_seen |= set(np.flatnonzero(state[..., 3].sum(axis=(0, 1))).tolist())
                    for k in seen:
                        seen[k] += counters[k]
            assert all(seen.values()), seen
            assert layers_seen == {0, 1, 4, 5, 6}, layers_seen
    finally:
        ds.close()


# ---------------------------------------------------------------- 4. orders, reset, a cull between steps, refusals
def test_orders_reset_and_a_cull_between_steps(device, host_scenes):
    lib = device
    hs, cam = host_scenes("cornell_box")
    W, H, spp = 24, 16, 3
    q = hs.params(W, spp, 8, seed=7, height=H)
    n = W * H * spp
    ds = DeviceScene(hs.desc)
    try:
        with ds.film(cam, q) as film, ds.splat(W, H, spp, filter=ffi.VK_SPLAT_TENT, radius=1.0) as sp, ds.robust(W, H, spp, buckets=2) as rb, \
                ds.lpe(W, H, spp, n) as acc, ds.paths(n) as pb:
            takers = {"film": lambda: film.deposit(pb), "splat": lambda: sp.deposit(pb), "robust": lambda: rb.deposit(pb),
                      "layers": lambda: acc.deposit(pb)}
            first = None
            for order in itertools.permutations(takers):
                for a in (film, sp, rb, acc):
                    a.reset()
                film.emit(pb, 0, 0, W, H, 0, spp)
                assert acc.step(pb, 100000).live == 0
                for who in order:
                    takers[who]()
                got = (film.debug_sums().tobytes(), sp.debug_sums().tobytes(), rb.debug_sums().tobytes(), acc.debug_sums().tobytes(),
                       bytes(film.info()), bytes(sp.info()), bytes(rb.info()), bytes(acc.info())[:72])
                first = first or got
                assert got == first, order
                # each has taken the batch: a second deposit of any is refused
                assert lib.vk_lpe_deposit(acc._h, pb._h) == ffi.VK_ERR_BAD_ARG
                assert b"deposited into a layer accumulator since its last begin or emit" in lib.vk_last_error()
                assert lib.vk_film_deposit(film._h, pb._h) == ffi.VK_ERR_BAD_ARG and lib.vk_robust_deposit(rb._h, pb._h) == ffi.VK_ERR_BAD_ARG
                assert lib.vk_splat_deposit(sp._h, pb._h, None) == ffi.VK_ERR_BAD_ARG
                assert acc.debug_sums().tobytes() == first[3]
            states, status = pb.results()
            sig, term = acc.tags(pb)
            want, counters = L.deposit(states, status, sig, term, standard_rules(), 7, 6, W, H, spp)
            assert np.array_equal(acc.debug_sums(), want) and L.counters_of(acc.info()) == counters
            assert np.array_equal(bits(acc.resolve()), bits(film.resolve(spp)))
            # reset zeroes sums and counters — not the tags, not the binding — and the accumulator takes the same frame again
            acc.reset()
            assert not acc.debug_sums().any() and acc.info().deposits == 0 and L.counters_of(acc.info()) == dict.fromkeys(L.COUNTERS, 0)
            assert np.array_equal(acc.tags(pb)[0], sig)
            rgb, share = acc.resolve(want_share=True)
            assert not rgb.any() and not share.any()
            film.emit(pb, 0, 0, W, H, 0, spp)
            assert acc.step(pb, 100000).live == 0
            acc.deposit(pb)
            assert np.array_equal(acc.debug_sums(), want) and acc.info().deposits == 1

            # vk_paths_cull between steps: a culled path keeps the tag of its last recorded bounce
            rays, st0 = emu_film_ffi.emit(cam, q, 0, 0, W, H, 0, spp)
            eb = emu_paths_ffi.Batch(hs.desc, **S.shade_kwargs(q, q.integrator, q.max_depth))
            eb.begin(rays, st0)
            tags = L.emulate(eb, n, max_bounces=2)
            film.emit(pb, 0, 0, W, H, 0, spp)
            assert acc.step(pb, 2).bounces == 2
            ids = pb.read()[0]
            assert np.array_equal(ids, eb.ids) and len(ids) > 10
            keep = (np.arange(len(ids)) % 3 != 0).astype(np.uint8)
            pb.cull(keep)
            eb.cull(keep)
            mid = acc.tags(pb)
            assert np.array_equal(mid[0], tags[0]) and np.array_equal(mid[1], tags[1])
            assert acc.step(pb, 100000).live == 0
            tags = L.emulate(eb, n, tags=tags, first_bounce=2)
            sig, term = acc.tags(pb)
            assert np.array_equal(sig, tags[0]) and np.array_equal(term, tags[1])
            gone = ids[keep == 0]
            assert np.array_equal(sig[gone], mid[0][gone]) and (pb.results()[1][gone] == ffi.VK_PATHS_CULLED).all()
            assert ((sig[gone] >> 8) & 0xFFFFF == 0).all() and ((sig[gone] >> 4) & 0xF == sig[gone] >> 28).all()
            acc.reset()
            acc.deposit(pb)
            states, status = pb.results()
            assert np.array_equal(acc.debug_sums(), L.deposit(states, status, sig, term, standard_rules(), 7, 6, W, H, spp)[0])
            lib.vk_lpe_destroy(None)
    finally:
        ds.close()


def test_refusals_leave_tracker_accumulator_and_batch_as_they_were(device, host_scenes):
    lib = device
    hs, cam = host_scenes("cornell_box")
    W, H = 24, 16
    q = hs.params(W, 1, 8, seed=9, height=H)
    n = W * H
    ds, other = DeviceScene(hs.desc), DeviceScene(hs.desc)
    try:
        h = C.c_void_p(0x77)
        arr = (ffi.LpeRule * 1)(lpe_rule(3))
        bad = ffi.LpeParams(3, 0, 1, 0, arr)
        assert lib.vk_lpe_create(ds._h, W, H, 1, n, C.byref(bad), C.byref(h)) == ffi.VK_ERR_BAD_ARG and b"layer is not below n_layers" in lib.vk_last_error()
        big = ffi.LpeParams(16, 0, 0, 0, None)
        assert lib.vk_lpe_create(ds._h, 8192, 8192, 1, n, C.byref(big), C.byref(h)) == ffi.VK_ERR_BAD_ARG and b"exceeds 2^27" in lib.vk_last_error()
        assert h.value == 0x77
        with ds.film(cam, q) as film, ds.lpe(W, H, 1, n) as acc, ds.lpe(W, H, 1, n) as second, ds.lpe(W, H, 1, 100) as small, \
                ds.paths(n) as pb, other.paths(n) as foreign, ds.paths(16) as never, ds.paths(100) as run, ds.paths(n) as plain:
            film.emit(pb, 0, 0, W, H, 0, 1)
            acc.step(pb, 100000)
            acc.deposit(pb)
            sums0, tags0 = acc.debug_sums().tobytes(), acc.tags(pb)
            info = ffi.PathsStepInfo()
            stamp = bytes(info)

            bound = [True]                     # whether acc is bound to pb's current begin: vk_lpe_tags answers only then

            def unchanged(batch, before, ai):
                assert bytes(batch.info()) == before and bytes(acc.info()) == ai and acc.debug_sums().tobytes() == sums0
                if bound[0]:
                    now = acc.tags(pb)
                    assert np.array_equal(now[0], tags0[0]) and np.array_equal(now[1], tags0[1])

            def refused(call, batch, word, tracker=None):
                tracker = tracker or acc
                before, ai = bytes(batch.info()), bytes(acc.info())
                sig = np.full(n, 7, u32)
                rc = {"step": lambda: lib.vk_lpe_step(tracker._h, batch._h, 1, C.byref(info)),
                      "step0": lambda: lib.vk_lpe_step(tracker._h, batch._h, 0, C.byref(info)),
                      "deposit": lambda: lib.vk_lpe_deposit(tracker._h, batch._h),
                      "tags": lambda: lib.vk_lpe_tags(tracker._h, batch._h, sig.ctypes.data, sig.ctypes.data)}[call]()
                assert rc == ffi.VK_ERR_BAD_ARG, (call, word)
                assert word in lib.vk_last_error(), (call, lib.vk_last_error())
                assert bytes(info) == stamp and (sig == 7).all()
                unchanged(batch, before, ai)

            refused("deposit", pb, b"deposited into a layer accumulator since its last begin or emit")
            for call in ("step", "deposit", "tags"):
                refused(call, foreign, b"belongs to another scene")
                refused(call, never, b"before vk_paths_begin or vk_film_emit")
            film.regen_begin(run, 0, 0, W, H, 0, 1)
            for call in ("step", "deposit", "tags"):
                refused(call, run, b"on a regenerating path batch")
            refused("step0", pb, b"max_bounces must be >= 1")
            # more started paths than the tracker's table holds
            film.emit(plain, 0, 0, W, H, 0, 1)
            for call in ("step", "deposit", "tags"):
                refused(call, plain, b"started more paths than the tracker's capacity", small)
            # a batch another tracker (or nobody) has stepped
            plain.step(1)
            assert plain.info().live > 0
            refused("step", plain, b"the tracker is not bound to it")
            refused("tags", plain, b"the tracker is not bound to the path batch")
            plain.step(100000)
            refused("deposit", plain, b"the tracker is not bound to the path batch")
            refused("tags", pb, b"the tracker is not bound to the path batch", second)
            # vk_paths_step in between: the tracker missed a bounce
            film.emit(pb, 0, 0, W, H, 0, 1)
            bound[0] = False
            refused("tags", pb, b"the tracker is not bound to the path batch")             # (a new emit is a new begin)
            assert acc.step(pb, 1).live > 0
            bound[0], tags0 = True, acc.tags(pb)
            refused("deposit", pb, b"live paths (step or cull them first)")
            pb.step(1)
            refused("step", pb, b"bounces the tracker did not record")
            pb.step(100000)
            refused("deposit", pb, b"bounces the tracker did not record")
            assert lib.vk_lpe_step(None, pb._h, 1, None) == ffi.VK_ERR_BAD_ARG and lib.vk_lpe_step(acc._h, None, 1, None) == ffi.VK_ERR_BAD_ARG
            img = np.full(W * H * 3, 7, f32)
            for layer, k, word in ((7, 1, b"layer must be below n_layers or VK_LPE_ALL"), (0xFFFFFFFE, 1, b"layer must be below"), (0, 0, b"n must be >= 1")):
                assert lib.vk_lpe_resolve(acc._h, layer, k, img.ctypes.data, None) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error()
            assert lib.vk_lpe_resolve(acc._h, 0, 1, None, img.ctypes.data) == ffi.VK_ERR_BAD_ARG and (img == 7).all()
            assert acc.debug_sums().tobytes() == sums0
            # the batch is as it was: emitted again and stepped by the tracker alone, it goes in
            film.emit(pb, 0, 0, W, H, 0, 1)
            acc.step(pb, 100000)
            acc.deposit(pb)
            assert acc.info().deposits == 2 and np.array_equal(acc.debug_sums(), 2 * np.frombuffer(sums0, np.int64).reshape(H, W, 7, 4))
    finally:
        other.close()
        ds.close()


# ---------------------------------------------------------------- 5. radiometry
SPHERE_D = (1, 2, 3, 4)


def sphere_rules():
    """layer k - 1: the lamp met on segment k — ENDED, last code EMIT, final depth k: emission ends a path before its depth moves
    (tests/test_lpe_emu.py), so k bounces leave state.depth at k —; the rest in layer 4"""
    return [lpe_rule(k - 1, 0xF0000000, ffi.VK_LPE_EMIT << 28, status=ENDED, depth=(k, k)) for k in SPHERE_D], len(SPHERE_D) + 1, len(SPHERE_D)


def test_layers_by_segment_meet_the_integrating_sphere(device):
    """radiometry_ref's integrating sphere, its 16 x 16 frame at 1024 samples per pixel and max_depth 50 in ONE run: the layers of the
    paths that met the lamp on segment 1 .. d, added up, are the frame within d segments — a (f Le) (1 - q^(d-1)) / (1 - q) —, for d = 1
    (exactly 0: no pixel sees the lamp), 2, 3 and 4.  Judged by radiometry_ref.check(): |z| <= 4 and SE <= 0.5 % of the value; the power
    control (one segment more) must be rejected at d = 2 and 3.  SE / want of the pixels' spread on the CPU emulators, largest channel:
    d = 2 0.33 %, d = 3 0.27 %, d = 4 0.27 % (this test's rules on tests/lpe_ref.py's emulated frame, 262 144 paths; z at most 2.0)."""
    cases = {d: R.sphere_frame(d) for d in SPHERE_D}
    full = R.sphere_frame(50)
    owner, desc = full.scene()
    p = full.render_params()
    W, H = full.size
    rules, n_layers, rest = sphere_rules()
    ds = DeviceScene(desc)
    try:
        with ds.film(full.cam, p) as film, ds.paths(W * H * 1024) as pb, ds.lpe(W, H, p.samples_per_pixel, W * H * 1024, rules, n_layers, rest) as acc:
            layers = acc.render(film, pb)
            assert np.array_equal(bits(acc.resolve()), bits(film.resolve()))
            assert acc.info().deposits == p.samples_per_pixel // 1024
        assert not layers[0].any()
        total = np.zeros((H, W, 3))
        for d in SPHERE_D:
            total = total + layers[d - 1].astype(np.float64)
            mean, se, z = cases[d].check_means(total, f"layers up to segment {d}")[0]
            print(f"\n   d = {d}: mean {mean} se {se} z {z}")
    finally:
        ds.close()
