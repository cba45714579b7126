"""Reconstruction filters against tests/splat_laws_ref.py, the operation in f64 written as a gather from its meaning (frame convention,
half-open support, the three published kernels) — on the CPU: tests/splat_ref.py's restatement of the header's operation list and the
host build of vk_splat.h (tests/emu) are each held to it, within the bound that module derives from the arithmetic.  a. random positions,
b. exact edges (dyadic positions and radii, membership pair for pair), c. reproduction laws on a symmetric lattice (constant, ramp, step
edge), d. the state's own position against where its camera ray went, e. a sparse frame under negative lobes.  First the closed form's own
self-tests, with no project code.  Run with -s for each test's worst deviation / bound and its marginal or unjudged share.

The builders below are shared with tests/test_gpu_splat_laws.py."""
import numpy as np
import pytest

import emu_splat_ffi as EMU
import film_ref as F
import geometry_ref as G
import splat_laws_ref as L
import splat_ref as R
from descs import Desc, camera, params
from vecchio_amd import ffi

f32, f64 = np.float32, np.float64
BOX, TENT, MITCHELL = L.BOX, L.TENT, L.MITCHELL
KIND_NAMES = {BOX: "box", TENT: "tent", MITCHELL: "mitchell"}
INTERIOR = (MITCHELL, 1.5, 0.25, 0.625)


def _settings():
    out = list(L.FILTERS)
    out += [(kind, r, R.THIRD if kind == MITCHELL else 0.0, R.THIRD if kind == MITCHELL else 0.0)
            for kind in (BOX, TENT, MITCHELL) for r in (0.5, 0.75, 1.25, 2.0)]
    out += [(MITCHELL, 2.0, b, c) for b, c in ((0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0))] + [INTERIOR]
    seen = []
    for sp in out:
        if sp not in seen:
            seen.append(sp)
    return seen


SETTINGS = _settings()
SETTING_IDS = [f"{KIND_NAMES[k]}{r:g}" + (f"-b{b:.3g}-c{c:.3g}" if k == MITCHELL else "") for k, r, b, c in SETTINGS]
CATMULL = (MITCHELL, 2.0, 0.0, 0.5)
SPP = 40
WORST = {}                                                  # kind name -> worst ratio of this run (printed by the last test)


def note(sp, ratio):
    k = KIND_NAMES[sp[0]]
    WORST[k] = max(WORST.get(k, 0.0), ratio)


def below(v):
    return np.nextafter(f32(v), f32(-1))


def radiances(n, seed):
    """(n, 3) float32 of both signs, well below the sums' clamp"""
    return np.random.default_rng(seed).uniform(-2.0, 4.0, (n, 3)).astype(f32)


def finished(acc, W, H):
    """hand-made finished states (tests/test_splat_emu.py's way) whose pixel lies outside the frame: with positions it is not read"""
    n = len(acc)
    return F.states_for(np.full(n, W * H + 5, np.uint32), acc), np.full(n, ffi.VK_PATHS_CULLED, np.uint32)


def random_positions(W, H, n, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 2)) * np.array([W, H])).astype(f32)
    return np.minimum(pos, np.array([below(W), below(H)], f32))


def lattice(W, H):
    """8 x 8 samples per pixel at (i + (2n + 1) / 16, j + (2m + 1) / 16): symmetric about every pixel centre, never on a support boundary
    of a radius that is a multiple of 1/4; in row order"""
    x = (np.arange(8 * W) * 2 + 1) / 16.0
    y = (np.arange(8 * H) * 2 + 1) / 16.0
    yy, xx = np.meshgrid(y, x, indexing="ij")
    return np.stack([xx.ravel(), yy.ravel()], axis=1).astype(f32)


CONSTANT = np.array([0.75, -1.5, 2.0], f32)
RAMP = np.array([[0.05, -0.11, 0.3], [-0.07, 0.02, 0.5], [0.013, 0.09, -1.0]])        # a, b, c of r, g, b: a x + b y + c, a != b


def ramp_at(x, y):
    return np.stack([RAMP[c, 0] * x + RAMP[c, 1] * y + RAMP[c, 2] for c in range(3)], axis=-1)


def lattice_radiances(pos, W):
    """name -> (n, 3) float32 on the lattice: a constant, a ramp and a step edge at a non-symmetric x"""
    x, y = pos[:, 0].astype(f64), pos[:, 1].astype(f64)
    edge = 0.4 * W + 0.3
    step = np.where((x < edge)[:, None], np.array([3.0, -0.5, 0.25]), np.array([-1.0, 2.0, 0.125]))
    return {"constant": np.tile(CONSTANT, (len(pos), 1)), "ramp": ramp_at(x, y).astype(f32), "step": step.astype(f32)}


def check_lattice(sp, W, H, name, acc, cf, image, what):
    """the reproduction laws on a resolved frame; returns the worst ratio"""
    worst, unjudged = L.assert_image(cf, image, what)
    assert unjudged == 0.0
    img = np.asarray(image, f64).reshape(H, W, 3)
    # what the f32 rounding of the radiances themselves may move an exact-arithmetic resolve by
    rounding = L.U * float(np.abs(acc).max()) * (cf.abs_weight / cf.sums[..., 3])[..., None] + 1e-13
    if name == "constant":
        dev = np.abs(img - CONSTANT.astype(f64)) / (cf.image_bound + rounding)
        worst = max(worst, float(dev.max()))
    if name == "ramp":
        r = f64(f32(sp[1]))
        X, Y = np.arange(W) + 0.5, np.arange(H) + 0.5
        inner = ((Y - r >= 0) & (Y + r <= H))[:, None] & ((X - r >= 0) & (X + r <= W))[None, :]
        want = ramp_at(*np.meshgrid(X, Y))
        dev = np.where(inner[..., None], np.abs(img - want) / (cf.image_bound + rounding), 0.0)
        worst = max(worst, float(dev.max()))
    assert worst <= 1.0, f"{what}: {name} is not reproduced, ratio {worst:.3g}"
    return worst


def sparse_case(W, H):
    """case e: as many samples as pixels, anywhere in the frame, under Catmull-Rom.  The seed is the first whose CLOSED FORM leaves at most
    MAX_UNJUDGED of the frame unjudged and, on a frame of a hundred pixels or more, gives some pixel a surely negative weight"""
    n = W * H
    for seed in range(200):
        pos = random_positions(W, H, n, seed=1000 * W + H + 7919 * seed)
        acc = radiances(n, seed + 5)
        cf = L.gather(CATMULL, pos, acc, W, H)
        negative = (cf.sums[..., 3] < -cf.bound[..., 3]).any()
        if (~cf.judged & ~cf.black).mean() <= L.MAX_UNJUDGED and (negative or n < 100):
            return pos, acc, cf
    raise AssertionError("no seed meets the cap")


ROLLED = dict(lookfrom=(3, 2, 5), lookat=(0.5, 0.2, -1), vup=(0.6, 0.8, 0.1), vfov=40.0, aspect=21.0 / 13.0, aperture=0.3, focus=4.5, t0=0.0,
              t1=1.0)
RAY_W, RAY_H, RAY_SPP, RAY_SEED = 21, 13, 3, 11
RAY_SETTINGS = [L.FILTERS[0], L.FILTERS[3], L.FILTERS[4], CATMULL]


def far_scene():
    """one small sphere far behind the camera: every camera ray misses"""
    d = Desc()
    s = d.sphere((30, 20, 50), 0.5, d.lambertian(0.5, 0.5, 0.5))
    return d, d.finish(d.big_box(s, s))


def rolled_camera():
    c = ROLLED
    return camera(c["lookfrom"], c["lookat"], c["vfov"], c["aspect"], c["aperture"], c["focus"], c["t0"], c["t1"], c["vup"])


def positions_of_rays(origin, direction, W, H):
    """Where a camera ray went, in frame coordinates, from the ray alone: origin + direction lies on the focus plane at lower_left +
    s horizontal + t vertical (geometry_ref.focus_point) whatever the lens offset; horizontal and vertical are orthogonal, so s and t are
    projections; px = s (width - 1), py = t (height - 1) (geometry_ref.pixel_st).  Returns ((n, 2) float32 inside the frame, (sx, sy):
    how far the true position may lie from it — geometry_ref.BOUND['camera'] of the focus distance on the plane, in pixels, plus the
    rounding to f32)."""
    c = ROLLED
    cam = G.camera_new(c["lookfrom"], c["lookat"], c["vup"], c["vfov"], c["aspect"], c["aperture"], c["focus"], c["t0"], c["t1"])
    rel = origin.astype(f64) + direction.astype(f64) - cam["lower_left_corner"]
    hor, ver = cam["horizontal"], cam["vertical"]
    px = rel @ hor / (hor @ hor) * (W - 1)
    py = rel @ ver / (ver @ ver) * (H - 1)
    slack = tuple(G.BOUND["camera"] * c["focus"] / np.linalg.norm(v) * (e - 1) + L.U * e for v, e in ((hor, W), (ver, H)))
    pos = np.stack([px, py], axis=1).astype(f32)
    return np.clip(pos, f32(0), np.array([below(W), below(H)], f32)), slack


def check_ray_positions(sp, W, H, acc, pos, slack, own, given, what):
    """own / given: (sums, contributions) of a deposit at the states' own positions and at `pos`.  Both within the closed form at `pos` —
    the first with the positions' slack — and so of each other; returns (worst ratio, marginal share)"""
    exact, loose = L.gather(sp, pos, acc, W, H), L.gather(sp, pos, acc, W, H, slack=slack)
    worst = max(L.assert_sums(exact, given[0], given[1], f"{what} given"), L.assert_sums(loose, own[0], own[1], f"{what} own"))
    apart = np.abs(own[0] - given[0]).astype(f64) * L.UNIT
    assert (apart <= exact.bound + loose.bound).all(), what
    return worst, loose.st.marginal_share()


# ================================================================ the closed form's own self-tests: no project code
BC = [(1.0 / 3.0, 1.0 / 3.0), (1.0, 0.0), (0.0, 0.5), (0.25, 0.625)]


def test_published_kernel_values():
    for (B, C), k0, k1 in zip(BC[:3], (8.0 / 9.0, 2.0 / 3.0, 1.0), (1.0 / 18.0, 1.0 / 6.0, 0.0)):
        assert abs(L.mitchell(B, C, 0.0) - k0) < 1e-15 and abs(L.mitchell(B, C, 1.0) - k1) < 1e-15 and abs(L.mitchell(B, C, -1.0) - k1) < 1e-15
    for B, C in BC + [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0)]:
        near, far, _, _ = L.mitchell_pieces(B, C)
        assert abs(L._poly(far, 2.0)) < 1e-15 and abs(L.mitchell_slope(B, C, 2.0, 1)) < 1e-15           # k(2) = k'(2) = 0
        assert abs(L._poly(near, 1.0) - L._poly(far, 1.0)) < 1e-15                                        # continuous at 1
        assert abs(L.mitchell_slope(B, C, 1.0, 0) - L.mitchell_slope(B, C, 1.0, 1)) < 1e-15
        assert abs(L.mitchell_slope(B, C, 1.0, 0) + (B / 2.0 + C)) < 1e-15
        assert L.mitchell(B, C, 2.0) == 0.0 and L.mitchell(B, C, 2.5) == 0.0 and L.mitchell(B, C, -3.0) == 0.0


def test_partitions_of_unity():
    x = np.random.default_rng(1).random(1000)
    worst = 0.0
    for B, C in BC:
        total = sum(L.mitchell(B, C, x + k) for k in range(-3, 3))
        worst = max(worst, float(np.abs(total - 1.0).max()))
    tent = sum(L.tent(x + k) for k in range(-2, 2))
    print(f"\n   partition of unity: Mitchell-Netravali {worst:.3g}, tent {np.abs(tent - 1.0).max():.3g}")
    assert worst < 1e-14 and np.abs(tent - 1.0).max() < 1e-15
    # the same through profile(): TENT at radius 1, MITCHELL at radius 2
    total = sum(L.profile((TENT, 1.0, 0, 0), x + k) * L.in_support((TENT, 1.0, 0, 0), x + k) for k in range(-2, 2))
    assert np.abs(total - 1.0).max() < 1e-15
    total = sum(L.profile((MITCHELL, 2.0, 0.5, 0.25), x + k) * L.in_support((MITCHELL, 2.0, 0.5, 0.25), x + k) for k in range(-3, 3))
    assert np.abs(total - 1.0).max() < 1e-14


def test_the_gather_by_hand():
    """one sample, TENT of radius 1.5, on a 4 x 3 frame: by hand"""
    cf = L.gather((TENT, 1.5, 0, 0), [[1.25, 0.5]], [[2.0, -1.0, 0.5]], 4, 3, members=True)
    wx = np.array([1 - 0.75 / 1.5, 1 - 0.25 / 1.5, 1 - 1.25 / 1.5, 0.0])          # centres 0.5, 1.5, 2.5; 3.5 is 2.25 away
    wy = np.array([1.0, 1 - 1.0 / 1.5, 0.0])                                      # centres 0.5, 1.5; 2.5 is 2 away
    assert np.allclose(cf.sums[..., 3], wy[:, None] * wx[None, :], atol=1e-15) and np.allclose(cf.sums[..., 1], -cf.sums[..., 3], atol=1e-15)
    assert cf.st.pairs == 6 and cf.st.marginal_pairs == 0 and cf.members[0].sum() == 6
    # d = -r is in, d = +r is out, and both are marginal
    edge = L.gather((BOX, 1.0, 0, 0), [[1.5, 0.5]], [[1.0, 1.0, 1.0]], 4, 1)
    assert edge.sums[0, :, 3].tolist() == [0.0, 1.0, 1.0, 0.0] and edge.st.marginal_triples == 2 and edge.st.marginal_pairs == 2


# ================================================================ a. random positions
@pytest.mark.parametrize("sp", SETTINGS, ids=SETTING_IDS)
def test_random_positions(sp, oracle):
    worst, share = 0.0, 0.0
    for W, H in L.FRAMES:
        n = SPP * W * H
        pos, acc = random_positions(W, H, n, seed=W * 100 + H), radiances(n, seed=W + H)
        cf = L.gather(sp, pos, acc, W, H)
        assert cf.st.marginal_share() <= L.MAX_MARGINAL and (cf.st.solid >= 1).all(), (sp, W, H)
        share = max(share, cf.st.marginal_share())
        states, status = finished(acc, W, H)
        for who, mod in (("restatement", R), ("emulator", EMU)):
            sums, counters = mod.deposit(states, status, W, H, SPP, sp, pos)
            assert counters["deposited"] == n
            worst = max(worst, L.assert_sums(cf, sums, counters["contributions"], f"{who} {sp} {W}x{H}"))
            worst = max(worst, L.assert_image(cf, R.resolve(sums), f"{who} {sp} {W}x{H}")[0])
    note(sp, worst)
    print(f"\n   random positions {sp}: worst deviation / bound {worst:.3g}, marginal triples {share:.2e}")


# ================================================================ b. exact edges
def dyadic_positions(W, H):
    """coordinates that are multiples of 1/16: every quarter of the first two pixels (d = -r and d = +r for every radius that is a multiple
    of 1/4, pixel corners, fx = 0), 1/16 and 15/16, the same in the middle and at the far edge; all four frame corners"""
    def axis(extent):
        v = [q / 4.0 for q in range(8)] + [1 / 16.0, 15 / 16.0]
        v += [extent // 2 + q / 4.0 for q in range(4)] + [extent - 1 + q for q in (0.0, 0.25, 0.5, 0.75, 15 / 16.0)]
        return sorted({x for x in v if 0 <= x < extent})
    xs, ys = axis(W), axis(H)
    pts = [(x, ys[(3 * i) % len(ys)]) for i, x in enumerate(xs)] + [(xs[(5 * j + 1) % len(xs)], y) for j, y in enumerate(ys)]
    far_x, far_y = W - 1 / 16.0, H - 1 / 16.0
    pts += [(0.0, 0.0), (far_x, 0.0), (0.0, far_y), (far_x, far_y), (W - 1.0, H - 1.0), (0.5, 0.5), (W - 0.5, H - 0.5)]
    return np.array(sorted(set(pts)), f32)


def nextafter_positions(W, H):
    """one float below the next pixel and below the frame's end: not dyadic"""
    return np.array([(below(1.0), below(1.0)), (below(W), below(H)), (below(W), 0.25), (0.25, below(H)), (below(1.0), 0.5)], f32)


@pytest.mark.parametrize("sp", [s for s in SETTINGS if s[1] in L.RADII], ids=[i for s, i in zip(SETTINGS, SETTING_IDS) if s[1] in L.RADII])
def test_exact_edges(sp, oracle):
    pairs = boundary = either = 0
    for W, H in L.FRAMES:
        dyadic, loose = dyadic_positions(W, H), nextafter_positions(W, H)
        pos = np.concatenate([dyadic, loose])
        assert (dyadic * 16 == np.round(dyadic * 16)).all()
        acc = radiances(len(pos), seed=3)
        cf = L.gather(sp, pos, acc, W, H, members=True)
        exact = L.gather(sp, dyadic, acc[:len(dyadic)], W, H)
        # nothing dyadic is within the band of a boundary without being ON it: on it, every f32 step is exact and the f64 rule decides
        d = np.concatenate([(dyadic[:, a].astype(f64)[:, None] - (np.arange(e) + 0.5)[None, :]).ravel() for a, e in ((0, W), (1, H))])
        off = np.abs(np.abs(d) - f64(f32(sp[1])))
        assert ((off == 0.0) | (off >= 1.0 / 16.0)).all() and exact.st.marginal_triples == int((off == 0.0).sum())
        states, status = finished(acc, W, H)
        for i in range(len(pos)):
            is_dyadic = i < len(dyadic)
            want = cf.members[i]
            maybe = np.zeros_like(want) if is_dyadic else cf.maybe[i]
            for who, mod in (("restatement", R), ("emulator", EMU)):
                sums, counters = mod.deposit(states[i:i + 1], status[i:i + 1], W, H, SPP, sp, pos[i:i + 1])
                what = f"{who} {sp} {W}x{H} at {pos[i].tolist()}"
                changed = sums[..., 3] != 0
                assert not (changed & ~want & ~maybe).any(), f"{what}: a pixel outside the support received weight"
                # a pixel of the support may stay unchanged only where its weight is below one unit of the sums (the far end of a tent)
                silent = want & ~changed & ~maybe
                assert (np.abs(cf.weights[i][silent]) < 2.0 * L.UNIT).all(), f"{what}: a pixel of the support received nothing"
                lo, hi = int((want & ~maybe).sum()), int((want | maybe).sum())
                assert lo <= counters["contributions"] <= hi, f"{what}: {counters['contributions']} contributions, {lo}..{hi} pairs"
            pairs += int(want.sum())
            either += int(maybe.sum())
        boundary += exact.st.marginal_triples
    assert boundary > 0 and pairs > 0
    print(f"\n   exact edges {sp}: {pairs} pairs matched one by one, {boundary} dyadic triples exactly on a boundary, "
          f"{either} pairs of the nextafter positions within the band")


# ================================================================ c. reproduction laws
@pytest.mark.parametrize("sp", [s for s in SETTINGS if s[1] in L.RADII], ids=[i for s, i in zip(SETTINGS, SETTING_IDS) if s[1] in L.RADII])
def test_reproduction_laws(sp, oracle):
    worst = 0.0
    for W, H in L.FRAMES:
        pos = lattice(W, H)
        for name, acc in lattice_radiances(pos, W).items():
            cf = L.gather(sp, pos, acc, W, H)
            assert cf.st.marginal_triples == 0 and cf.judged.all(), (sp, W, H, name)
            states, status = finished(acc, W, H)
            for who, mod in (("restatement", R), ("emulator", EMU)):
                sums, counters = mod.deposit(states, status, W, H, 64, sp, pos)
                what = f"{who} {sp} {W}x{H} {name}"
                worst = max(worst, L.assert_sums(cf, sums, counters["contributions"], what))
                worst = max(worst, check_lattice(sp, W, H, name, acc, cf, R.resolve(sums), what))
    note(sp, worst)
    print(f"\n   reproduction laws {sp}: worst deviation / bound {worst:.3g}, nothing marginal, nothing unjudged")


# ================================================================ d. the state's own position
@pytest.mark.parametrize("sp", RAY_SETTINGS, ids=["box0.5", "tent1.5", "mitchell", "catmull"])
def test_the_states_own_position_is_where_its_ray_went(sp, oracle):
    W, H, spp = RAY_W, RAY_H, RAY_SPP
    _, desc = far_scene()
    p = params(W, H, spp, seed=RAY_SEED, integrator=ffi.VK_INTEGRATOR_SCATTER)
    fh = oracle.first_hits(desc, rolled_camera(), p, 0, spp)
    pixel, sample = F.ids_of(W, 0, 0, W, H, 0, spp)
    n = len(pixel)
    pos, slack = positions_of_rays(fh["origin"].reshape(n, 3), fh["direction"].reshape(n, 3), W, H)
    # the rays do land in their pixels: the recovery is no restatement of the jitter
    assert (np.abs(pos[:, 0] - (pixel % W + 0.5)) <= 0.5 + slack[0]).all() and (np.abs(pos[:, 1] - (pixel // W + 0.5)) <= 0.5 + slack[1]).all()
    acc = radiances(n, seed=9)
    states = F.states_for(pixel, acc, seed=RAY_SEED)
    states["sample"] = sample
    status = np.full(n, ffi.VK_SHADE_MISS, np.uint32)
    worst = share = 0.0
    for who, mod in (("restatement", R), ("emulator", EMU)):
        own, oc = mod.deposit(states, status, W, H, spp, sp)
        given, gc = mod.deposit(states, status, W, H, spp, sp, pos)
        assert oc["deposited"] == gc["deposited"] == n
        w, share = check_ray_positions(sp, W, H, acc, pos, slack, (own, oc["contributions"]), (given, gc["contributions"]), f"{who} {sp}")
        worst = max(worst, w)
        # and the position stated outright: pixel corner + draws 0 and 1
        direct = L.gather(sp, L.positions_of_states(pixel, R.jitter(states["seed"], pixel, sample), W), acc, W, H)
        worst = max(worst, L.assert_sums(direct, own, oc["contributions"], f"{who} {sp} draws"))
    note(sp, worst)
    print(f"\n   own positions {sp}: worst deviation / bound {worst:.3g}; positions known to {slack[0]:.2e}, {slack[1]:.2e} px, "
          f"marginal triples under that slack {share:.2e}")


# ================================================================ e. sparse, negative lobes
@pytest.mark.parametrize("frame", L.FRAMES, ids=[f"{w}x{h}" for w, h in L.FRAMES])
def test_sparse_negative_lobes(frame, oracle):
    W, H = frame
    pos, acc, cf = sparse_case(W, H)
    unjudged = float((~cf.judged & ~cf.black).mean())
    assert unjudged <= L.MAX_UNJUDGED
    states, status = finished(acc, W, H)
    worst = 0.0
    for who, mod in (("restatement", R), ("emulator", EMU)):
        sums, counters = mod.deposit(states, status, W, H, 1, CATMULL, pos)
        worst = max(worst, L.assert_sums(cf, sums, counters["contributions"], f"{who} {W}x{H}"))
        worst = max(worst, L.assert_image(cf, R.resolve(sums), f"{who} {W}x{H}")[0])
    note(CATMULL, worst)
    print(f"\n   sparse Catmull-Rom {W}x{H}: worst deviation / bound {worst:.3g}, unjudged {unjudged:.3f}, "
          f"black by negative weight {int((cf.sums[..., 3] < -cf.bound[..., 3]).sum())} pixels")


def test_worst_ratios_of_this_run():
    print("\n   worst deviation / bound per kind, CPU: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
