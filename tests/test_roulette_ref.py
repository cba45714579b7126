"""The termination rule of a path batch handle (vk_roulette_set) on the CPU: tests/roulette_ref.py's draw against the oracle's
stream, its q on hand-made throughputs at every edge of the definition, the depth gate, and — on the emulators' batch loop — that the
rule leaves the frame's mean where it was while the same rule without its scale does not (the test's own power).  This pins the
reference tests/test_gpu_roulette.py holds the device against."""
import numpy as np
import pytest

import roulette_ref as RR
from vecchio_amd import ffi
from vecchio_amd.scene import PATH_STATE_DTYPE

f32 = np.float32


def test_draw_is_the_oracles_stream(oracle):
    for seed, pixel, sample in ((0, 0, 0), (0xC0FFEE12345, 7, 3), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE)):
        want = oracle.draws(seed ^ RR.SALT, pixel, sample, 0, 60)
        depth = np.arange(1, 61)
        got = RR.draw(np.full(60, seed, np.uint64), np.full(60, pixel, np.uint32), np.full(60, sample, np.uint32), depth)
        assert got.dtype == f32 and got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (seed, pixel, sample)
        for d in (1, 2, 59):                    # the header's terms, one depth at a time
            assert oracle.draws(seed ^ RR.SALT, pixel, sample, 0, d)[d - 1] == RR.draw(seed, pixel, sample, d)
        assert ((got >= 0) & (got < 1)).all() and len(set(got.tolist())) == 60


def states_with(thr, depth, seed=11):
    thr = np.asarray(thr, f32).reshape(-1, 3)
    s = np.zeros(len(thr), PATH_STATE_DTYPE)
    s["thr"], s["depth"] = thr, depth
    s["seed"], s["pixel"], s["sample"] = seed, np.arange(len(thr)), 5
    return s


@pytest.mark.parametrize("first_depth,q_min,q_max", RR.RULES + ((2, 0.25, 0.25), (2, 2.0 ** -24, 1.0)))
def test_q_on_hand_made_throughputs(first_depth, q_min, q_max):
    names, thr, want = RR.edge_throughputs(q_min, q_max)
    assert {"nan_in_one", "nan_in_all", "plus_inf", "zero", "negative", "denormal", "max_at_q_min", "max_at_q_max"} <= set(names)
    q = RR.q_of(thr, q_min, q_max)
    assert q.dtype == f32
    for k, name in enumerate(names):
        assert q[k].view(np.uint32) == want[k].view(np.uint32), (name, thr[k], q[k], want[k])
        assert f32(q_min) <= q[k] <= f32(q_max), name
        # exactly q_min, q_max or the maximum of the components that are numbers
        finite_max = np.fmax.reduce(thr[k])
        assert q[k] in (f32(q_min), f32(q_max)) or q[k] == finite_max, name
    # the decision and the scale follow from q and the draw alone
    for depth in (first_depth, first_depth + 9):
        s = states_with(thr, depth)
        keep, scale = RR.rule(s, first_depth, q_min, q_max)
        u = RR.draw(s["seed"], s["pixel"], s["sample"], s["depth"])
        assert keep.dtype == np.uint8 and scale.dtype == f32
        assert keep.tolist() == (u < want).astype(np.uint8).tolist()
        assert scale.view(np.uint32).tolist() == (f32(1.0) / want).astype(f32).view(np.uint32).tolist()
    if q_max == 1.0:                            # q == 1: the throughput stays bit for bit
        k = names.index("above_q_max")
        assert want[k] == f32(1.0) and RR.rule(states_with(thr[k], first_depth), first_depth, q_min, q_max)[1][0].view(np.uint32) == 0x3F800000


@pytest.mark.parametrize("first_depth,q_min,q_max", RR.RULES)
def test_the_depth_gate(first_depth, q_min, q_max):
    n = 4096
    thr = np.full((n, 3), 1e-3, f32)            # q = q_min: most draws end the path where the rule applies
    below, at = states_with(thr, first_depth - 1), states_with(thr, first_depth)
    keep, scale = RR.rule(below, first_depth, q_min, q_max)
    assert keep.all() and (scale == 1).all()
    keep, scale = RR.rule(at, first_depth, q_min, q_max)
    share = keep.mean()
    assert abs(share - q_min) < 5 * np.sqrt(q_min * (1 - q_min) / n) and (scale == f32(1.0) / f32(q_min)).all()
    # apply(): only SCATTERED records at or beyond first_depth change, in the status word or in thr
    from vecchio_amd.scene import SHADED_DTYPE
    items = np.zeros(2 * n, SHADED_DTYPE)
    items["state"] = np.concatenate([below, at])
    items["status"] = np.resize(np.array([ffi.VK_SHADE_SCATTERED, ffi.VK_SHADE_ENDED, ffi.VK_SHADE_MISS], np.uint32), 2 * n)
    out = RR.apply(items, first_depth, q_min, q_max)
    touched = (items["status"] == ffi.VK_SHADE_SCATTERED) & (items["state"]["depth"] >= first_depth)
    assert out[~touched].tobytes() == items[~touched].tobytes()
    culled = out["status"] == ffi.VK_PATHS_CULLED
    assert culled.any() and not (culled & ~touched).any() and out["state"][culled].tobytes() == items["state"][culled].tobytes()
    went_on = touched & ~culled
    assert went_on.any() and (out["state"]["thr"][went_on] == (f32(1e-3) * (f32(1.0) / f32(q_min)))).all()


# ---------------------------------------------------------------- unbiasedness, and the test's own power
def emu_frame(desc, cam, q, rule=None, scaled=True):
    """acc per path of the whole frame on the emulators' batch loop, the rule applied after every bounce through Batch.cull"""
    import emu_film_ffi
    import emu_paths_ffi
    import shade_ref as S
    rays, states = emu_film_ffi.emit(cam, q, 0, 0, q.width, q.height, 0, q.samples_per_pixel)
    b = emu_paths_ffi.Batch(desc, **S.shade_kwargs(q, q.integrator, q.max_depth))
    b.begin(rays, states)
    walked = bounces = 0
    while b.live:
        walked, bounces = walked + b.live, bounces + 1
        b.step()
        if rule is not None and b.live:
            keep, scale = RR.rule(b.states, *rule)
            b.cull(keep, scale if scaled else None)
    return b.results()[0]["acc"], walked, bounces, int(b.retired[ffi.VK_PATHS_CULLED])


def test_the_rule_is_unbiased_and_the_test_would_see_a_bias(built, host_scenes):
    U = RR.UNBIASED
    hs, cam = host_scenes(U["scene"])
    frame = lambda seed: hs.params(U["width"], U["spp"], U["max_depth"], seed=seed, height=U["height"])
    plain, walked0, bounces0, culled0 = emu_frame(hs.desc, cam, frame(U["seed_plain"]))
    ruled, walked1, bounces1, culled1 = emu_frame(hs.desc, cam, frame(U["seed_rule"]), U["rule"])
    control, _, _, _ = emu_frame(hs.desc, cam, frame(U["seed_control"]), U["rule"], scaled=False)
    assert len(plain) == len(ruled) == len(control) == U["width"] * U["height"] * U["spp"] == 262144
    z, zc = RR.channel_z(plain, ruled), RR.channel_z(plain, control)
    print(f"rays walked {walked0} -> {walked1}, bounces {bounces0} -> {bounces1}, culled {culled1}; |z| {z}, control |z| {zc}")
    assert culled0 == 0 and culled1 > 1000 and walked1 < walked0
    assert max(z) <= U["z_max"], z
    assert min(zc) >= U["z_control_min"], zc
