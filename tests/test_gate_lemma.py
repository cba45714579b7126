"""The gate lemma of exact re-treeing (vk_trace.h segment_unsafe, vk_linearize.h rt_unit_growth), attacked.

Exact re-treeing walks a tree rebuilt over the reference's leaf units and claims the result of BVHNode::hit on the tree as handed over
(accel.rs:58-83).  The claim rests on the rebuilt tree's gates being SOUND: whenever the reference could have accepted a sphere — its
unit's box passes (accel.rs:60) and Sphere::hit reports a root (hittable.rs:65-95) — the rebuilt walk must test that sphere as long as
its closest hit so far is farther.  In exact arithmetic a hit lies on its sphere, inside its box, behind the box's entry, and any gate
works; in f32 a hit can lie off the sphere by eta = 32 u (rho + R)^2 / R and precede the entry of a long unit's box by the box's length.
  * part A measures the constant (the forward error analysis gives < 30; the lemma uses 32);
  * part B aims rays at the worst configuration (grazing the sphere where it touches its box, nearly parallel to that face, long units)
    and checks the gate itself: the GROWN gates of the proven form never fail, the bare ones of the empirical form do;
  * part C builds a scene around one such ray: the empirical form returns the WRONG sphere (that is why it is opt-in,
    VK_SCENE_EMPIRICAL_TREES), the default returns the reference's;
  * part D (round 5) REFUTES the shortcut "gate every sphere by its OWN box grown by the lemma's growth" (docs/gate_lemma.md section 6):
    from hundreds of radii away Sphere::hit reports roots for lines that miss the sphere's grown own box altogether, and the reference,
    whose unit box such a line does pass, accepts them.
"""
import ctypes as C
import os

import numpy as np
import pytest

from descs import Desc, camera, params
from vecchio_amd import ffi


@pytest.fixture(scope="module")
def lem(emu, built):
    import emu_ffi
    lib = emu_ffi.load()
    lib.emu_lemma_residual.restype = C.c_double
    lib.emu_lemma_residual.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    lib.emu_gate_soundness.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_float, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    lib.emu_hit.argtypes = [C.POINTER(ffi.SceneDesc), ffi.F3, ffi.F3, C.POINTER(C.c_float * 3)]
    lib.emu_own_gate_soundness.argtypes = [C.c_uint64, C.c_uint64, C.c_float, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    lib.emu_near_form_claims.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    lib.emu_own_gate_ray.argtypes = [C.c_float * 3, C.c_float, C.c_float * 3, C.c_float * 3, C.c_float, C.c_double, C.POINTER(C.c_float)]
    return lib


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sphere_hit_points_lie_within_eta_of_the_sphere(seed, lem):
    """|dist(o + t d, centre) - R| <= K u (rho + R)^2 / R for every root Sphere::hit can report: K over 2 M configurations (origins
    inside, on and up to 10^4 radii away; grazing and head-on; radii 1e-3 .. 1e5) and 200 k steps of bit-level hill climbing."""
    k = lem.emu_lemma_residual(2_000_000, seed, 200_000)
    print(f"seed {seed}: largest K = {k:.2f} (the lemma's constant: 32)")
    assert 1.0 < k < 16.0


def soundness(lem, grow, pad, r0, n=1_500_000, seed=7):
    cnt = (C.c_uint64 * 2)()
    v = (C.c_float * 19)()
    lem.emu_gate_soundness(n, seed, grow, pad, r0, cnt, v)
    return int(cnt[0]), int(cnt[1]), np.array(list(v), np.float32)


@pytest.mark.parametrize("pad,r0", [(0.25, 2000.0), (0.25, 60.0), (0.0625, 2000.0), (0.5, 500.0)])
def test_grown_gates_are_sound(pad, r0, lem):
    cases, failed, _ = soundness(lem, 1, pad, r0)
    print(f"padding {pad}, trusted ball {r0}: {cases} rays the reference can accept, {failed} gate failures")
    assert cases > 100_000 and failed == 0


def test_bare_gates_are_not(lem):
    """the empirical form's gate (the unit's box as handed over): fails on rays of this kind at every padding — less often at 1/16 than
    at 1/256, which is what the seed sweeps of round 3 saw from the other side"""
    f256 = soundness(lem, 0, 1.0 / 256.0, 2000.0)
    f16 = soundness(lem, 0, 1.0 / 16.0, 2000.0)
    print(f"bare gates: {f256[1]} of {f256[0]} fail at 1/256, {f16[1]} of {f16[0]} at 1/16")
    assert f256[1] > f16[1] > 0


# ---- part C: a scene around one failing ray (found by part B at padding 1/16: a unit of two spheres 115 apart; the ray comes from 38
# units away, passes 4e-5 above the first sphere's top, where it touches its box, descending 3.5e-7 per unit: Sphere::hit reports a hit
# at t = 1.24, the ray enters the unit's box at t = 4.82).  Every component of its direction is above the 1e-6 below which the kernel
# does not trust its fast box test anyway (vk_trace.h set_space).  Z is hit at t = 2.0 and sits in a unit with a larger box, so the
# rebuilt tree visits it first.
RAY_O = (-38.24720001220703, 0.40005257725715637, -0.03297411650419235)
RAY_D = (30.9495906829834, -1.0907649993896484e-05, 0.01718575693666935)
RAY_LLC = (-7.297609329223633, 0.4000416696071625, -0.015788359567523003)      # RAY_O + RAY_D: f32(RAY_LLC - RAY_O) == RAY_D
T_X, T_Z = 1.2354214191436768, 2.000


def adversarial_scene():
    f32 = np.float32
    d = Desc()
    grey = d.lambertian(.5, .5, .5)
    red, green = d.light(1, 0, 0), d.light(0, 1, 0)          # (emitters: a sample's colour says which sphere won)

    def own(c, r):
        c = np.array(c, f32)
        return c - f32(r), c + f32(r)

    def unit(a, b):                                          # a BVHNode of two spheres, box = surrounding_box (accel.rs:117-131)
        ra, rb = d.sphere(a[0], a[1], a[2]), d.sphere(b[0], b[1], b[2])
        ba, bb = own(a[0], a[1]), own(b[0], b[1])
        bx = np.minimum(ba[0], bb[0]), np.maximum(ba[1], bb[1])
        return d.bvh_node(ra, rb, tuple(bx[0]), tuple(bx[1])), bx

    def join(x, y):
        bx = np.minimum(x[1][0], y[1][0]), np.maximum(x[1][1], y[1][1])
        return d.bvh_node(x[0], y[0], tuple(bx[0]), tuple(bx[1])), bx

    A = unit(((0.0, 0.2, 0.0), 0.2, red), ((114.64096069335938, 0.2, -0.5463153123855591), 0.2, grey))
    B = unit(((23.74, 0.45, 0.0), 0.1, green), ((23.74, 0.2, 400.0), 0.2, grey))
    nodes = [unit(((k * 3.0, -60.0, 5.0), 0.2, grey), ((k * 3.0 + 1.0, -60.0, 5.5), 0.2, grey)) for k in range(16)]
    while len(nodes) > 1:
        nodes.append(join(nodes.pop(0), nodes.pop(0)))
    world = join(join(A, B), nodes[0])                       # the reference visits A first: T = inf, the unit passes, X is accepted
    return d, d.finish(world[0])


def emu_hit(lem, desc, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        out = (C.c_float * 3)()
        assert lem.emu_hit(desc, ffi.F3(*RAY_O), ffi.F3(*RAY_D), C.byref(out)) == 0
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return float(out[0]), int(np.float32(out[1]).view(np.uint32)) & ffi.VK_REF_INDEX_MASK, bool(out[2])


@pytest.mark.parametrize("variant", ["0", "1"])
def test_the_constructed_ray(variant, lem, oracle):
    d, desc = adversarial_scene()
    h = oracle.hit(desc, RAY_O, RAY_D)
    assert h is not None and abs(h["t"] - T_X) < 1e-5          # the reference's answer: sphere X, early by a factor of four
    # the default: a world with a unit too long for a grown gate is not rebuilt (vk_linearize.cpp rt_grow_units): walked as handed over
    t, prim, _ = emu_hit(lem, desc, EMU_GLOBAL_VARIANT=variant)
    assert (t, prim) == (h["t"], 0)
    desc.contents.flags = ffi.VK_SCENE_REFERENCE_TREE
    assert emu_hit(lem, desc, EMU_GLOBAL_VARIANT=variant)[:2] == (h["t"], 0)
    # the empirical form (every unit rebuilt with its bare box), as the device runs scenes from global memory: Z first, then X's unit
    # does not pass T (1 + 1/16): WRONG
    desc.contents.flags = ffi.VK_SCENE_EMPIRICAL_TREES
    t, prim, redone = emu_hit(lem, desc, EMU_GLOBAL_VARIANT=variant, VK_GATE_PROOF="0")
    # (in both of the device's forms.  Until the safe-winner test got its exact second level — the reference's own AxisBB::hit of the
    # winner's box where the fast arithmetic's margin is inconclusive — the LDS form, whose fused box test has a margin that grows
    # with |o / d|, called every winner of a ray this close to parallel to an axis unsafe and was right by accident.)
    assert prim == 2 and abs(t - T_Z) < 1e-2 and not redone


def window_setup(flags):
    """64 x 64 primary rays within 4e-7 rad of the constructed one (scatter integrator: a sample is the colour of what it hit)"""
    d, desc = adversarial_scene()
    desc.contents.flags = flags
    # a camera whose pixel row t looks along RAY_D + (0, (t - 1/2) 2e-5, 0) (main.rs:115-119).  The hit on X is a rounding accident of
    # Sphere::hit, so x and z of the direction must be RAY_D's to the bit: part B only reports rays with f32(llc - o) == d.
    f32 = np.float32
    o, llc = np.array(RAY_O, f32), np.array(RAY_LLC, f32)
    assert tuple(float(x) for x in (llc - o)) == RAY_D
    cam = ffi.Camera()
    cam.origin = ffi.F3(*o); cam.lower_left_corner = ffi.F3(llc[0], f32(np.float64(llc[1]) - 1.0e-5), llc[2])
    cam.horizontal = ffi.F3(0, 0, 0); cam.vertical = ffi.F3(0, 2.0e-5, 0)
    cam.u = ffi.F3(0, 0, 1); cam.v = ffi.F3(0, 1, 0); cam.w = ffi.F3(-1, 0, 0)
    cam.lens_radius = 0.0; cam.time0 = 0.0; cam.time1 = 1.0
    p = params(64, 64, 1, max_depth=2, seed=3, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SKY)
    return d, desc, cam, p


def render_window(variant_env, flags, emu, oracle, monkeypatch):
    d, desc, cam, p = window_setup(flags)
    for k, v in variant_env.items():
        monkeypatch.setenv(k, v)
    img_o, ps_o = oracle.render_samples(desc, cam, p)
    img_e, ps_e, _, _ = emu.render_samples(desc, cam, p)
    return ps_o, ps_e


def test_a_window_of_rays_around_it(emu, oracle, built, monkeypatch):
    ps_o, ps_e = render_window({"EMU_GLOBAL_VARIANT": "1"}, 0, emu, oracle, monkeypatch)
    assert np.array_equal(ps_o[:, :3], ps_e[:, :3])
    red = int((ps_o[:, 0] == 1.0).sum())
    assert red > 50, "the window does not see the early hits on X"
    ps_o, ps_e = render_window({"EMU_GLOBAL_VARIANT": "1", "VK_GATE_PROOF": "0"}, ffi.VK_SCENE_EMPIRICAL_TREES, emu, oracle, monkeypatch)
    wrong = int((ps_o[:, :3] != ps_e[:, :3]).any(axis=1).sum())
    print(f"{red} of 4096 rays hit X in the reference; the empirical form gets {wrong} of them wrong")
    assert wrong > 0


# ---- part D: gates made of the spheres' OWN boxes are not sound (the refutation of VERDICT r4's item 1, docs/gate_lemma.md section 6)
def test_own_box_gates_are_not_sound(lem):
    """A sphere's own box grown by rt_unit_growth (d* = sqrt 3 (R + g): growth 5e-4 R) is passed by every ray whose hit point lies
    within the growth of the box or precedes the ray's ENTRY into it — but a line that passes a 0.2-sphere at 1.15 radii from 450 units
    away never enters that box, and the f32 quadratic still reports a root for it.  The reference's unit box (a leaf's box around TWO
    spheres) is what such a line passes; gating by it is what round 4 proves, and what stays."""
    for r0 in (500.0, 2000.0, 20000.0):
        cnt = (C.c_uint64 * 2)(); v = (C.c_float * 12)()
        lem.emu_own_gate_soundness(400_000, 3, 0.25, r0, cnt, v)
        print(f"trusted ball {r0}: {cnt[0]} rays with a candidate, own-box gate closed for {cnt[1]}; worst: the line misses the sphere by "
              f"{v[11]:.2f} radii from {np.linalg.norm(np.array(v[4:7]) - np.array(v[0:3])):.0f} away")
        assert cnt[0] > 50_000 and cnt[1] > 100


def test_the_ray_that_refuted_them(lem):
    """found on the 1 M-sphere stress scene (emulator, 96 x 54 x 2 spp: 14 of 18 432 samples differed from the tree as handed over with
    own-box gates): a PRIMARY ray, 446.7 from sphere 284 099, whose line passes the centre at 0.2301 = 1.15 R (exact arithmetic) — 0.228 in
    z alone, outside the grown own box — and for which Sphere::hit reports t = 41.5557; the reference's walk, whose boxes the ray passes,
    takes that hit, the own-box walk returned the ground sphere at t = 41.7669."""
    f3 = C.c_float * 3
    out = (C.c_float * 4)()
    rc = lem.emu_own_gate_ray(f3(-224.58372497558594, 0.20000000298023224, 87.19125366210938), 0.20000000298023224,
                              f3(206.818161, 109.090912, 47.727272), f3(-10.3778687, -2.61903381, 0.954879761), 0.25, 20000.0, out)
    assert rc == 0
    has, t, passes, growth = list(out)
    assert has == 1.0 and abs(t - 41.5557022) < 1e-4 and passes == 0.0 and 1e-4 < growth < 1e-3


# ---- part E: the NEAR form (round 5; vk_linearize.cpp rt_grow_near, docs/gate_lemma.md section 7).  Own-box gates are sound for origins
# NEAR the sphere (part D refutes them for far ones); a segment's result is taken only if its hit lies within `reach` of its origin, or
# if the ray runs clear of every small sphere beyond that — the two conditions under which no far sphere can hold a closer candidate.
@pytest.mark.parametrize("mode,what", [(0, "near gates closed"), (1, "candidates of far spheres within reach"),
                                       (2, "candidates of far spheres under a ray that tested clear")])
def test_near_form_claims(mode, what, lem):
    total = [0, 0]
    for seed in (1, 2, 3):
        cnt = (C.c_uint64 * 2)(); v = (C.c_float * 12)()
        lem.emu_near_form_claims(mode, 1_500_000, seed, cnt, v)
        total[0] += cnt[0]; total[1] += cnt[1]
        assert cnt[1] == 0, f"{what}: {cnt[1]} of {cnt[0]}, e.g. centre {list(v[0:3])} R {v[3]} o {list(v[4:7])} d {list(v[7:10])} t {v[10]} rho_near {v[11]}"
    print(f"{what}: 0 of {total[0]}")
    assert total[0] > 200_000


def test_the_clearance_margin_is_not_idle(lem):
    """control of mode 2: rays that dip a quarter of a radius INTO the box around the spheres' surfaces do find candidates"""
    cnt = (C.c_uint64 * 2)(); v = (C.c_float * 12)()
    lem.emu_near_form_claims(3, 1_500_000, 1, cnt, v)
    print(f"a quarter of a radius inside the box: {cnt[1]} candidates in {cnt[0]} pairs")
    assert cnt[1] > 100
    # ... and so do rays that merely stay outside the box itself (M = 0): the margin is needed, and the rays above sit on its boundary
    lem.emu_near_form_claims(4, 500_000, 1, cnt, v)
    print(f"no margin at all: {cnt[1]} candidates in {cnt[0]} pairs")
    assert cnt[1] > 100


# ---- part F: the GRID form (late round 5; vk_linearize.cpp rt_build_grid, vk_trace.h grid_step, docs/gate_lemma.md section 8) finds
# every candidate: its closest hit is the closest hit over ALL spheres, for rays from on, in, near and far from the spheres, along the
# layer, and past spheres where the f32 discriminant reports hits that are not there.
@pytest.mark.parametrize("scene,n", [("random_spheres_iow", 600_000), ("stress_spheres:60", 100_000), ("stress_spheres:150", 15_000)])
def test_grid_form_finds_every_candidate(scene, n, lem, monkeypatch):
    from vecchio_amd import HostScene
    lem.emu_grid_claims.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    monkeypatch.delenv("EMU_GRID_NO_DILATION", raising=False)
    hs = HostScene(scene, 1)
    total = 0
    for seed in (1, 2):
        cnt = (C.c_uint64 * 3)(); v = (C.c_float * 8)()
        assert lem.emu_grid_claims(hs.desc, n, seed, cnt, v) == 0
        assert cnt[2] == 0, f"{scene}: {cnt[2]} of {cnt[0]} rays, e.g. o {list(v[0:3])} d {list(v[3:6])} grid {v[6]} all spheres {v[7]}"
        assert cnt[1] > 0.5 * cnt[0]
        total += cnt[0]
    print(f"{scene}: 0 of {total} rays")


def test_the_grids_dilation_is_not_idle(lem, monkeypatch):
    """control of part F: with the dilation switched off (the cells on the ray's exact path only) candidates ARE missed — hits an f32
    Sphere::hit reports for rays that pass a far sphere at more than its radius"""
    from vecchio_amd import HostScene
    lem.emu_grid_claims.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    monkeypatch.setenv("EMU_GRID_NO_DILATION", "1")
    hs = HostScene("stress_spheres:60", 1)
    cnt = (C.c_uint64 * 3)(); v = (C.c_float * 8)()
    assert lem.emu_grid_claims(hs.desc, 150_000, 1, cnt, v) == 0
    print(f"no dilation: {cnt[2]} of {cnt[0]} rays differ")
    assert cnt[2] > 20


# The large spheres' common gate, against large spheres FAR from the layer.  A world of the grid form: a 10 x 10 layer of r = 0.2 spheres
# at pitch 1, a ground sphere, and one large sphere (2.5 .. 64 median radii: behind the common gate) 2 000 or 10 000 from the layer.  From
# an origin near the layer such a sphere's false roots lie up to b (rho + R) from it, three orders of magnitude beyond any dilation
# measured at the layer; the gate must be dilated by the gated spheres' OWN distance and radius.  The same sphere standing in the layer is
# the control every version of the gate passed.
FAR_SPHERES = {"r0.6_at_2000": ((2000.0, 0.6, 5.0), 0.6), "r2_at_10000": ((10000.0, 2.0, 5.0), 2.0), "r0.6_in_the_layer": ((5.0, 0.6, 5.0), 0.6)}


def far_sphere_claims(lem, which, n, seed):
    from test_retree import far_sphere_world
    lem.emu_grid_claims.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    g, desc = far_sphere_world(*FAR_SPHERES[which])
    cnt = (C.c_uint64 * 3)(); v = (C.c_float * 8)()
    assert lem.emu_grid_claims(desc, n, seed, cnt, v) == 0, "not a world the grid form applies to"
    return cnt, v


@pytest.mark.parametrize("which", sorted(FAR_SPHERES))
def test_the_large_spheres_gate_holds_for_spheres_far_from_the_layer(which, lem, monkeypatch):
    for k in ("EMU_GRID_NO_DILATION", "EMU_GRID_NO_GATE_DILATION", "EMU_GRID"):
        monkeypatch.delenv(k, raising=False)
    for seed in (1, 2):
        cnt, v = far_sphere_claims(lem, which, 400_000, seed)
        assert cnt[2] == 0, f"{which}: {cnt[2]} of {cnt[0]} rays, e.g. o {list(v[0:3])} d {list(v[3:6])} grid {v[6]} all spheres {v[7]}"
        assert cnt[1] > 0.5 * cnt[0]
        print(f"{which} seed {seed}: 0 of {cnt[0]} rays ({cnt[1]} with a hit)")


def test_the_large_spheres_gate_dilation_is_not_idle(lem, monkeypatch):
    """control of the test above: with the common gate's dilation switched off (the box around the large spheres as it stands) the far
    spheres' candidates ARE missed"""
    monkeypatch.delenv("EMU_GRID_NO_DILATION", raising=False)
    monkeypatch.setenv("EMU_GRID_NO_GATE_DILATION", "1")
    for which in ("r0.6_at_2000", "r2_at_10000"):
        cnt, v = far_sphere_claims(lem, which, 400_000, 1)
        print(f"{which}, no gate dilation: {cnt[2]} of {cnt[0]} rays differ")
        assert cnt[2] > 20
