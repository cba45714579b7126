"""Russian roulette on the device (vk_roulette_set).  1. The count pass's second form alone, through vk_debug_compact_roulette, at
every size of the compaction's own test and on records with the rule's edge throughputs, against tests/roulette_ref.py followed by
tests/paths_ref.py, on every output byte.  2. THE CONTRACT on every scene of the shade tests' set and each integrator vk_render allows
there: a batch stepped with the rule set is, after every bounce and at its end, byte for byte the batch stepped with the rule off that
gets vk_paths_read, the rule in numpy and vk_paths_cull after each bounce.  3. The same for regenerating runs of awkward capacities: sums,
counters, the resolved frame, every bounce's live paths, any slicing.  4. The rule leaves the frame's mean where it was, and the same rule
without its scale does not.  5. The setting: the handle's, kept, changed mid-run, refused without a trace.  6. No side effect on vk_render,
the launch log or a vk_progress handle."""
import ctypes as C

import numpy as np
import pytest

import paths_ref as P
import roulette_ref as RR
import shade_ref as S
import test_gpu_film as GF
import test_roulette_abi as RA
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu
SPP = 3
ALL = 0xFFFFFFFF
bits, frame_params = GF.bits, GF.frame_params
CULLED = ffi.VK_PATHS_CULLED


def same_live(a, b, what):
    """vk_paths_read of two batches, byte for byte"""
    for name, g, w in zip(("ids", "rays", "states"), a, b):
        assert g.tobytes() == w.tobytes(), f"{what}: {name} differ"


def host_rule(rule, cull, scaled=True):
    """the rule from the host, for a batch after a bounce: cull(batch, keep, scale)"""
    def between(batch):
        _, _, states = batch.read()
        keep, scale = RR.rule(states, *rule)
        cull(batch, keep, scale if scaled else None)
    return between


def as_set(rule):
    """a rule as PathBatch.roulette() returns it: the two bounds rounded to f32"""
    return (rule[0], float(np.float32(rule[1])), float(np.float32(rule[2])))


def counters(film):
    i = film.info()
    return (i.emitted, i.deposited, i.dropped, i.clamped, i.skipped)


def finished(info):
    return info.live == 0 and info.remaining == 0


# ---------------------------------------------------------------- 1. the kernel alone
@pytest.fixture(scope="module")
def any_scene(device, host_scenes):
    desc, _, _ = S.scene("builder", "cornell_box", host_scenes)
    ds = DeviceScene(desc)
    yield ds
    ds.close()


@pytest.mark.parametrize("n", P.SIZES)
def test_count_pass_against_the_reference(n, any_scene):
    patterns = P.patterns(n)
    patterns["wild"] = np.random.default_rng(n).integers(0, 8, n).astype(np.uint32)          # statuses above 4 too
    decided = 0
    for rule in RR.RULES:
        for name, status in patterns.items():
            what = f"n {n}, {name}, rule {rule}"
            items, ids, n_ids = RR.edge_items(status, *rule)
            before = items.copy()
            got = any_scene.debug_compact_paths(items, ids, n_ids, canary=P.CANARY, roulette=rule)
            after = RR.apply(items, *rule)
            P.assert_same(got, P.compact(after, ids, n_ids), what)
            assert items.tobytes() == before.tobytes(), what                                  # the caller's records are not rewritten
            decided += int((after["status"] != items["status"]).sum())
            # with q_max = 1 a path that goes on at q == 1 keeps its throughput's bits; everything the rule does not apply to is untouched
            alone = (items["status"] != ffi.VK_SHADE_SCATTERED) | (items["state"]["depth"] < rule[0])
            assert after[alone].tobytes() == items[alone].tobytes(), what
    assert decided > 0 or n < 8


def test_count_pass_of_nothing_and_its_refusals(any_scene):
    items, ids, n_ids = RR.edge_items(P.patterns(4)["all"], *RR.RULES[0])
    assert [int(c) for c in any_scene.debug_compact_paths(items[:0], ids[:0], n_ids, roulette=RR.RULES[0])[5]] == [0] * 5
    with pytest.raises(RuntimeError, match="an id is not below n_ids"):
        any_scene.debug_compact_paths(items, ids, int(ids.max()), roulette=RR.RULES[0])
    with pytest.raises(RuntimeError, match="first_depth must be >= 2"):
        any_scene.debug_compact_paths(items, ids, n_ids, roulette=(1, 0.1, 0.8))
    # the rule's q at its bounds: every record at q_min with a draw below it goes on, scaled by 1 / q_min exactly
    rule = (2, 0.25, 0.25)
    items["status"], items["state"]["depth"] = ffi.VK_SHADE_SCATTERED, 2
    got = any_scene.debug_compact_paths(items, ids, n_ids, roulette=rule)
    P.assert_same(got, P.compact(RR.apply(items, *rule), ids, n_ids), "q_min == q_max")


# ---------------------------------------------------------------- 2. THE CONTRACT
@pytest.mark.parametrize("kind,name", S.ALL_SCENES, ids=[f"{k}-{n}" for k, n in S.ALL_SCENES])
def test_contract_on_scene(kind, name, device, host_scenes):
    desc, cam, p = S.scene(kind, name, host_scenes)
    W, H = p.width, p.height
    n = W * H * SPP
    if (kind, name) == ("builder", "final_scene"):
        assert desc.contents.n_media > 0
    ds = DeviceScene(desc)
    culled = 0
    try:
        with ds.paths(n) as dev, ds.paths(n) as host:
            for integrator in S.integrators(desc):
                for depth in S.DEPTHS:
                    with ds.film(cam, frame_params(p, integrator, SPP, depth)) as film:
                        for rule in RR.RULES:
                            what = f"{kind} {name}, integrator {integrator}, max_depth {depth}, rule {rule}"
                            between = host_rule(rule, lambda b, keep, scale: b.cull(keep, scale))
                            dev.set_roulette(*rule)
                            assert host.roulette() is None
                            film.emit(dev, 0, 0, W, H, 0, SPP)
                            film.emit(host, 0, 0, W, H, 0, SPP)
                            k = 0
                            while dev.info().live:
                                a, b = dev.step(1), host.step(1)
                                assert a.bounces == 1 and a.kernel_launches == 5 and a.kernel_ms > 0, what
                                assert (a.traced, a.missed, a.ended, a.bad) == (b.traced, b.missed, b.ended, b.bad), (what, k)
                                if b.live:
                                    between(host)
                                assert a.live == dev.info().live == host.info().live, (what, k)
                                same_live(dev.read(), host.read(), f"{what}, bounce {k}")
                                k += 1
                            assert host.info().live == 0 and 1 <= k <= depth, what
                            (sa, ta), (sb, tb) = dev.results(), host.results()
                            assert sa.tobytes() == sb.tobytes() and ta.tobytes() == tb.tobytes(), what
                            assert bytes(dev.info()) == bytes(host.info()), what
                            inf = dev.info()
                            assert inf.retired[CULLED] == int((ta == CULLED).sum()) and sum(inf.retired) == n and inf.retired[1] == 0, what
                            culled += inf.retired[CULLED]
        if name in ("final_scene", "cornell_box"):
            assert culled > 100, (name, culled)
    finally:
        ds.close()


# ---------------------------------------------------------------- 3. regenerating runs
@pytest.mark.parametrize("name", ["cornell_box", "final_scene"])
def test_regenerating_runs(name, device, host_scenes):
    desc, cam, p = S.scene("builder", name, host_scenes)
    q = frame_params(p, spp=SPP, max_depth=50)
    W, H = q.width, q.height
    win = (0, 0, W, H, 0, SPP)
    ds = DeviceScene(desc)
    try:
        plain, _ = ds.render(cam, q)
        with ds.film(cam, q) as fa, ds.film(cam, q) as fb:
            for rule in RR.RULES:
                between = host_rule(rule, lambda b, keep, scale: fb.regen_cull(b, keep, scale))
                want = None
                for cap in (64, 65, 257, 773):
                    what = f"{name}, rule {rule}, capacity {cap}"
                    with ds.paths(cap) as dev, ds.paths(cap) as host:
                        fa.reset()
                        fb.reset()
                        img_b = fb.render_regen(host, cull=between, roulette=None)
                        img_a = fa.render_regen(dev, roulette=rule)
                        assert dev.roulette() == as_set(rule) and host.roulette() is None
                        assert fa.debug_sums().tobytes() == fb.debug_sums().tobytes(), what
                        assert counters(fa) == counters(fb) and np.array_equal(bits(img_a), bits(img_b)), what
                        assert bytes(dev.info()) == bytes(host.info()) and dev.info().retired[CULLED] > 0, what
                        assert not np.array_equal(bits(img_a), bits(plain)), what
                        # the frame does not depend on the capacity: a path's fate is a function of its own state
                        want = want or fa.debug_sums().tobytes()
                        assert fa.debug_sums().tobytes() == want, what
                        if cap in (65, 257):
                            # every bounce
                            fa.reset()
                            fb.reset()
                            fa.regen_begin(dev, *win)
                            fb.regen_begin(host, *win)
                            k = 0
                            while True:
                                a, b = fa.regen_step(dev, 1), fb.regen_step(host, 1)
                                assert a.bounces == 1 and a.kernel_launches == (6 if a.emitted else 5), (what, k)
                                assert (a.traced, a.emitted, a.remaining, a.missed, a.ended, a.bad) == \
                                    (b.traced, b.emitted, b.remaining, b.missed, b.ended, b.bad), (what, k)
                                if b.live:
                                    between(host)
                                assert a.live == host.info().live, (what, k)
                                same_live(dev.read(), host.read(), f"{what}, bounce {k}")
                                k += 1
                                if finished(a):
                                    break
                            assert fa.debug_sums().tobytes() == want == fb.debug_sums().tobytes() and counters(fa) == counters(fb), what
                        # any slicing
                        seen = []
                        for max_bounces in (1, 3, 1000):
                            fa.reset()
                            fa.regen_begin(dev, *win)
                            infos = [fa.regen_step(dev, max_bounces)]
                            while not finished(infos[-1]):
                                infos.append(fa.regen_step(dev, max_bounces))
                            assert fa.debug_sums().tobytes() == want, (what, max_bounces)
                            seen.append((bytes(dev.info()), sum(i.traced for i in infos), sum(i.kernel_launches for i in infos), counters(fa)))
                        assert seen[0] == seen[1] == seen[2], what
    finally:
        ds.close()


# ---------------------------------------------------------------- 4. unbiasedness, and the test's own power
def test_the_rule_is_unbiased_and_the_test_would_see_a_bias(device, host_scenes):
    U = RR.UNBIASED
    hs, cam = host_scenes(U["scene"])
    n = U["width"] * U["height"] * U["spp"]
    assert n == 2 ** 18
    ds = DeviceScene(hs.desc)
    try:
        with ds.paths(2 ** 18) as pb:
            def frame(seed, rule=None, between=None):
                q = hs.params(U["width"], U["spp"], U["max_depth"], seed=seed, height=U["height"])
                pb.set_roulette(*(rule or (None,)))
                with ds.film(cam, q) as film:
                    film.emit(pb, 0, 0, q.width, q.height, 0, q.samples_per_pixel)
                    traced = 0
                    while pb.info().live:
                        st = pb.step(1 if between else ALL)
                        traced += st.traced
                        if between and st.live:
                            between(pb)
                return pb.results()[0]["acc"].copy(), traced, pb.info().retired[CULLED]

            plain, t0, c0 = frame(U["seed_plain"])
            ruled, t1, c1 = frame(U["seed_rule"], U["rule"])
            # the control: the same rule through vk_paths_cull with scale = NULL
            control, _, c2 = frame(U["seed_control"], None, host_rule(U["rule"], lambda b, keep, scale: b.cull(keep, scale), scaled=False))
        z, zc = RR.channel_z(plain, ruled), RR.channel_z(plain, control)
        print(f"rays walked {t0} -> {t1}, culled {c1}; |z| {z}, control |z| {zc}")
        assert c0 == 0 and c1 > 1000 and c2 > 1000 and t1 < t0
        assert max(z) <= U["z_max"], z
        assert min(zc) >= U["z_control_min"], zc
    finally:
        ds.close()


# ---------------------------------------------------------------- 5. the setting
def test_the_setting_is_the_handles(device, host_scenes):
    lib = device
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    q = frame_params(p, spp=SPP, max_depth=20)
    W, H = q.width, q.height
    n = W * H * SPP
    rays = S.rays_of(cam)
    rule, other = RR.RULES
    ds = DeviceScene(desc)
    try:
        frame, _ = ds.render(cam, q)
        with ds.film(cam, q) as film, ds.paths(n) as pb, ds.paths(n) as ref, ds.paths(100) as small:
            # off after create; kept across begin, emit and regen_begin
            assert pb.roulette() is None and small.roulette() is None
            rp, on = ffi.RouletteParams(9, 9.0, 9.0, 9), C.c_int(7)
            assert lib.vk_roulette_get(pb._h, C.byref(rp), C.byref(on)) == ffi.VK_OK and on.value == 0 and bytes(rp) == bytes(16)
            for r in RA.ACCEPTED:
                pb.set_roulette(*r)
                assert pb.roulette() == as_set(r), r
            pb.set_roulette(*rule)
            from vecchio_amd.scene import make_path_states
            pb.begin(rays, make_path_states(len(rays), S.SEED, S.FIRST, 0), **S.shade_kwargs(q, q.integrator, 20))
            assert pb.roulette() == as_set(rule)
            pb.step(3)
            film.emit(pb, 0, 0, W, H, 0, SPP)
            assert pb.roulette() == as_set(rule)
            film.regen_begin(pb, 0, 0, W, H, 0, SPP)
            film.regen_step(pb, 2)
            assert pb.roulette() == as_set(rule) and ref.roulette() is None
            # every refusal leaves the getter's answer as it was, with the rule on and with it off
            for h, state in ((pb, as_set(rule)), (ref, None)):
                for fields, word in RA.REFUSALS:
                    bad = ffi.RouletteParams(*fields)
                    assert lib.vk_roulette_set(h._h, C.byref(bad)) == ffi.VK_ERR_BAD_ARG, fields
                    assert word in lib.vk_last_error(), (fields, lib.vk_last_error())
                    assert h.roulette() == state, fields
            # two runs with the rule give the same bytes
            film.reset()
            first = film.render_regen(small, roulette=rule)
            sums = film.debug_sums().tobytes()
            film.reset()
            assert np.array_equal(bits(film.render_regen(small)), bits(first)) and film.debug_sums().tobytes() == sums
            assert small.roulette() == as_set(rule) and small.info().retired[CULLED] > 0 and not np.array_equal(bits(first), bits(frame))
            # set_roulette(None) after use: vk_render's frame, bit for bit
            film.reset()
            assert np.array_equal(bits(film.render_regen(small, roulette=None)), bits(frame)) and small.roulette() is None
            assert small.info().retired[CULLED] == 0
            film.reset()
            assert np.array_equal(bits(film.render(pb, roulette=None)), bits(frame))
            # a change mid-run holds from the next bounce: off for two bounces, `rule` for two, `other` for two, off again
            plan = [None, None, rule, rule, other, other] + [None] * 50
            film.reset()
            film.emit(pb, 0, 0, W, H, 0, SPP)
            film.emit(ref, 0, 0, W, H, 0, SPP)
            k = 0
            while pb.info().live:
                pb.set_roulette(*(plan[k] or (None,)))
                st = pb.step(1)
                assert st.kernel_launches == 5
                if ref.step(1).live and plan[k]:
                    host_rule(plan[k], lambda b, keep, scale: b.cull(keep, scale))(ref)
                same_live(pb.read(), ref.read(), f"bounce {k}")
                k += 1
            assert k > 6 and pb.info().retired[CULLED] > 0 and bytes(pb.info()) == bytes(ref.info())
            assert pb.results()[0].tobytes() == ref.results()[0].tobytes() and pb.results()[1].tobytes() == ref.results()[1].tobytes()
            # two batches on one scene, one with the rule and one without, stepped alternately
            want_ruled = pb.results()
            film.emit(ref, 0, 0, W, H, 0, SPP)
            ref.step(ALL)
            want_plain = ref.results()
            assert np.isin(want_plain[1], (ffi.VK_SHADE_MISS, ffi.VK_SHADE_ENDED)).all()
            film.emit(pb, 0, 0, W, H, 0, SPP)
            film.emit(ref, 0, 0, W, H, 0, SPP)
            k = 0
            while pb.info().live or ref.info().live:
                pb.set_roulette(*(plan[k] or (None,)))
                pb.step(1)
                ref.step(2)
                k += 1
            for got, want in ((pb.results(), want_ruled), (ref.results(), want_plain)):
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    finally:
        ds.close()


# ---------------------------------------------------------------- 6. scene state
def test_the_rule_leaves_the_render_the_launch_log_and_a_progress_handle_alone(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    p = hs.params(96, 4, 20, seed=3)
    fq = hs.params(24, SPP, 20, seed=4, height=16)
    ds = DeviceScene(hs.desc)
    try:
        before, _ = ds.render(cam, p)
        ms, requeued = ds.last_kernel_ms(), ds.last_requeued_samples()
        launches = [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)]
        with ds.film(cam, fq) as film, ds.paths(100) as pb:
            film.render_regen(pb, roulette=RR.RULES[0])
            first = film.debug_sums().copy()
            assert pb.info().retired[CULLED] > 0
            assert abs(ds.last_kernel_ms() - ms) < 1e-4 and ds.last_requeued_samples() == requeued
            assert [bytes(l) for l in ffi.last_launches(ds._lib, ds._h)] == launches and launches
            after, _ = ds.render(cam, p)
            np.testing.assert_array_equal(bits(before), bits(after))
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
    finally:
        ds.close()
