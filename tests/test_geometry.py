"""First hits, media, textures and camera rays of the oracle and of the emulator against tests/geometry_ref.py: f64 closed forms written
from the reference's lines alone.  Every other geometry test holds the oracle and vk_trace.h to each other; a misreading the two share
(a rotation sense, the `1 -` of Sphere::spherical, the flip of ImageTexture's v, MovingSphere::center outside the shutter, an inclusive
bound) passes them all and fails here.  tests/test_gpu_geometry.py runs the same scenes and rays on the device.

Run with -s for the oracle's worst deviation from the f64 values per scene (what geometry_ref.MEASURED holds) and the excluded share of
every scene."""
import math

import numpy as np
import pytest

import geometry_ref as G
import rays_ref
from descs import Desc, camera, params
from test_fuzz_scenes import Gen, _corners
from vecchio_amd import ffi
from vecchio_amd.scene import make_rays

f32, f64 = np.float32, np.float64
SEED = 0xC0FFEE12345


@pytest.fixture(scope="session")
def emu_rays(built):
    import emu_rays_ffi
    emu_rays_ffi.load()
    return emu_rays_ffi


# ================================================================ random graphs
class GenNoMedia(Gen):
    """test_fuzz_scenes.Gen with a sphere wherever it would make a medium: a ConstantMedium draws from the ray's stream in the order the
    tree is walked, which a reference without a tree cannot follow (the media have their own test below)"""

    def medium(self):
        return self.sphere()


class Wild(Gen):
    """What Gen does not reach: rotations about all three axes by 40 to 175 degrees either way, chains of 1 to 6 wrappers, a Rotate
    directly over a Translate and the reverse, flipped lists, a Boxy under a rotation, negative radii, moving spheres whose shutter
    (0.3, 0.7) lies inside the camera's (0, 1) — rays meet them below time0, inside and above time1 —, nested and touching spheres, and
    (inside_points) ray origins inside a sphere and inside a Boxy.  About 24 objects under a random tree with real boxes."""

    def __init__(self, seed):
        super().__init__(seed)
        self.inside_points = []

    def moving(self):
        c0 = self.pos(); c1 = c0 + self.r.uniform(-0.7, 0.7, 3); rad = float(self.r.uniform(0.3, 0.8))
        t0, t1 = 0.3, 0.7
        at = lambda t: c0 + (c1 - c0) * ((t - t0) / (t1 - t0))            # the box covers the centre of every time in (0, 1)
        lo, hi = np.minimum(at(0.0), at(1.0)), np.maximum(at(0.0), at(1.0))
        return self.d.moving_sphere(tuple(c0), tuple(c1), t0, t1, rad, self.mat()), (lo - rad - 1e-3, hi + rad + 1e-3)

    def rotated(self, ref, bb, axis=None, deg=None):
        axis = int(self.r.integers(0, 3)) if axis is None else axis
        deg = float(self.r.uniform(40, 175) * self.r.choice([-1, 1])) if deg is None else deg
        ref = self.d.rotate(ref, axis, deg)
        a = np.deg2rad(deg); c, s = np.cos(a), np.sin(a)
        P = _corners(bb)
        i, j = [(1, 2), (0, 2), (0, 1)][axis]
        Q1, Q2 = P.copy(), P.copy()                                      # both senses: the box only has to contain the object
        Q1[:, i], Q1[:, j] = c * P[:, i] - s * P[:, j], s * P[:, i] + c * P[:, j]
        Q2[:, i], Q2[:, j] = c * P[:, i] + s * P[:, j], -s * P[:, i] + c * P[:, j]
        Q = np.concatenate([Q1, Q2])
        return ref, (Q.min(0) - 1e-2, Q.max(0) + 1e-2)

    def translated(self, ref, bb):
        off = self.r.uniform(-1.5, 1.5, 3)
        return self.d.translate(ref, tuple(off)), (bb[0] + off, bb[1] + off)

    def chain(self, ref, bb, n):
        for _ in range(n):
            ref, bb = self.translated(ref, bb) if self.r.uniform() < 0.5 else self.rotated(ref, bb)
            if self.r.uniform() < 0.15:
                ref = Desc.flip(ref)
        return ref, bb

    def small(self):
        """an object near the origin, so that a rotation of any angle keeps it within reach of the camera after a Translate"""
        k = int(self.r.integers(0, 4))
        c = self.r.uniform(-1.0, 1.0, 3)
        if k == 0:
            rad = float(self.r.uniform(0.4, 1.0)) * float(self.r.choice([-1, 1]))
            return self.d.sphere(tuple(c), rad, self.mat()), (c - abs(rad) - 1e-3, c + abs(rad) + 1e-3)
        if k == 1:
            p1 = c + self.r.uniform(0.5, 1.5, 3)
            return self.d.boxy(tuple(c), tuple(p1), self.mat()), (c - 1e-3, p1 + 1e-3)
        if k == 2:
            items, bb = [], None
            for _ in range(3):
                cc = c + self.r.uniform(-0.8, 0.8, 3); rad = float(self.r.uniform(0.3, 0.6))
                ref = self.d.sphere(tuple(cc), rad, self.mat())
                items.append(Desc.flip(ref) if self.r.uniform() < 0.5 else ref)
                b = (cc - rad - 1e-3, cc + rad + 1e-3)
                bb = b if bb is None else (np.minimum(bb[0], b[0]), np.maximum(bb[1], b[1]))
            return Desc.flip(self.d.list_(items)), bb
        s = self.r.uniform(0.5, 1.2, 2)
        ax = [(0, 1, 2), (0, 2, 1), (1, 2, 0)][int(self.r.integers(0, 3))]
        lo, hi = np.zeros(3), np.zeros(3)
        lo[ax[0]], hi[ax[0]], lo[ax[1]], hi[ax[1]] = c[ax[0]] - s[0], c[ax[0]] + s[0], c[ax[1]] - s[1], c[ax[1]] + s[1]
        lo[ax[2]], hi[ax[2]] = c[ax[2]] - 1e-3, c[ax[2]] + 1e-3
        return self.d.rect(float(lo[ax[0]]), float(hi[ax[0]]), float(lo[ax[1]]), float(hi[ax[1]]), float(c[ax[2]]), ax, self.mat()), (lo, hi)

    def placed(self, ref, bb):
        """a last Translate to somewhere in the camera's view"""
        off = self.pos() - (bb[0] + bb[1]) / 2
        return self.d.translate(ref, tuple(off)), (bb[0] + off, bb[1] + off)

    def build(self):
        objs = []
        # nested, touching and negative-radius spheres
        c, m = self.pos(), self.mat()
        objs.append((self.d.sphere(tuple(c), 1.5, self.surface[4]), (c - 1.6, c + 1.6)))
        objs.append((self.d.sphere(tuple(c), -1.3, self.surface[4]), (c - 1.4, c + 1.4)))
        objs.append((self.d.sphere(tuple(c), 0.5, m), (c - 0.6, c + 0.6)))
        self.inside_points.append((c, 0.4)); self.inside_points.append((c + [0.9, 0, 0], 0.3))
        c = self.pos()
        for off in (0.0, 1.6):                                   # two spheres of radius 0.8 that touch at one point
            cc = c + [off, 0, 0]
            objs.append((self.d.sphere(tuple(cc), 0.8, self.mat()), (cc - 0.9, cc + 0.9)))
        for _ in range(3):
            objs.append(self.moving())
        p0 = self.pos(); p1 = p0 + self.r.uniform(1.0, 2.0, 3)
        objs.append((self.d.boxy(tuple(p0), tuple(p1), self.mat()), (p0 - 1e-3, p1 + 1e-3)))
        self.inside_points.append(((p0 + p1) / 2, 0.3))
        for _ in range(2):
            objs.append(self.rect())
        # a Rotate directly over a Translate, and the reverse; each axis at least once
        for axis in range(3):
            ref, bb = self.small()
            ref, bb = self.translated(ref, bb)
            objs.append(self.placed(*self.rotated(ref, bb, axis)))
            ref, bb = self.small()
            ref, bb = self.rotated(ref, bb, axis)
            objs.append(self.placed(ref, bb))
        # chains of 1 to 6 wrappers over spheres, Boxys, flipped lists and rects
        for n in (1, 2, 3, 4, 5, 6, 6):
            ref, bb = self.chain(*self.small(), n)
            objs.append(self.placed(ref, bb))
        order = self.r.permutation(len(objs))
        world, _ = self.tree([objs[i] for i in order])
        desc = self.d.finish(world, [])
        ang = self.r.uniform(0, 6.28)
        cam = camera((5 + 11 * np.cos(ang), self.r.uniform(3, 8), 5 + 11 * np.sin(ang)), (5, 5, 5), vfov=50.0, aperture=0.0)
        p = params(20, 16, 1, max_depth=2, seed=int(self.r.integers(1, 1000)), integrator=ffi.VK_INTEGRATOR_SCATTER,
                   background=ffi.VK_BACKGROUND_SKY)
        return desc, cam, p


SCENES = [("gen", s) for s in (1001, 1018, 1026, 1031, 1038)] + [("wild", s) for s in (1, 2, 3, 4)]
WIDTH, HEIGHT = 60, 56
_cache = {}


def scene(kind, seed, oracle):
    """(generator, desc, cam, p, rays, where, f64 scene, f64 hits, stability record), built once"""
    key = (kind, seed)
    if key not in _cache:
        g = (GenNoMedia if kind == "gen" else Wild)(seed)
        desc, cam, p = g.build()
        if kind == "gen":                                       # Gen's few objects fill a seventh of its 50 degree view: look closer
            cam = camera(list(cam.origin), (5, 5, 5), vfov=30.0, aperture=0.0)
        p.width, p.height, p.samples_per_pixel = WIDTH, HEIGHT, 1
        sets = rays_ref.ray_sets(oracle, desc, cam, p)
        # the cut sets of rays_ref put tmax ON a hit and its neighbours, and its odd set holds NaN and zero rays: unstable by design
        known = sets.pop("tmax_cuts", None)
        sets.pop("odd", None)
        if known is not None:                                   # tmax one per cent before and after a known hit instead
            h = known[:len(known) // 3]
            t = rays_ref.ref_hits(oracle, desc, h, SEED, 0)["t"]
            sets["cuts"] = np.concatenate([make_rays(h["origin"], h["direction"], h["time"], t * f32(k)) for k in (0.99, 1.01)])
        rng = np.random.default_rng(seed)
        pts = getattr(g, "inside_points", [])
        if pts:
            o = np.concatenate([f32(c) + f32(r) * rng.uniform(-1, 1, (32, 3)).astype(f32) for c, r in pts])
            dd = rng.normal(size=(len(o), 3)).astype(f32) * rng.uniform(0.2, 5.0, (len(o), 1)).astype(f32)
            sets["inside_objects"] = make_rays(o, dd, rng.uniform(0, 1, len(o)))
        rays, where = rays_ref.all_rays(sets)
        assert len(rays) <= 4096
        sc = G.Scene(desc)
        want, record = G.reference(sc, rays)
        _cache[key] = (g, desc, cam, p, rays, where, sc, want, record)
    return _cache[key]


@pytest.mark.parametrize("kind,seed", SCENES, ids=[f"{k}-{s}" for k, s in SCENES])
def test_random_graph(kind, seed, oracle, emu_rays):
    g, desc, cam, p, rays, where, sc, want, record = scene(kind, seed, oracle)
    got = rays_ref.ref_hits(oracle, desc, rays, SEED, 7)
    worst = G.compare_hits(got, want, record, rays, f"oracle {kind} {seed}")
    print(f"\n   {kind} {seed}: {len(rays)} rays, {worst['hits']} stable hits, excluded {worst['excluded']:.4%}; oracle - f64: "
          + ", ".join(f"{k} {worst[k]:.3g}" for k in ("t", "p", "normal", "uv")))
    G.assert_within(worst, f"oracle {kind} {seed}")
    emu, _ = emu_rays.trace_rays(desc, rays, SEED, 7)
    G.assert_within(G.compare_hits(emu, want, record, rays, f"emulator {kind} {seed}"), f"emulator {kind} {seed}")
    assert want["hit"][where["primary"]].mean() > 0.2


def test_the_generators_reach_what_they_claim(oracle):
    """over the wild scenes: all three axes beyond 40 degrees, chains of 6, Rotate over Translate and the reverse, flipped lists, a Boxy
    face and a negative radius among the winners, moving spheres hit below, inside and above their shutter, origins inside objects"""
    axes, longest, pairs, winners, times = set(), 0, set(), set(), set()
    for kind, seed in SCENES:
        if kind != "wild":
            continue
        g, desc, cam, p, rays, where, sc, want, record = scene(kind, seed, oracle)
        axes |= {a for _, a, s, c in sc.rotates if abs(c) < math.cos(math.radians(40))}
        kind_of = lambda ref: ref >> 28

        def depth(ref):
            k, i = kind_of(ref), ref & G.INDEX_MASK
            if k == ffi.VK_KIND_TRANSLATE:
                pairs.add(("T", kind_of(sc.translates[i][0])))
                return 1 + depth(sc.translates[i][0])
            if k == ffi.VK_KIND_ROTATE:
                pairs.add(("R", kind_of(sc.rotates[i][0])))
                return 1 + depth(sc.rotates[i][0])
            return 0
        longest = max([longest] + [depth(ffi.make_ref(ffi.VK_KIND_TRANSLATE, i)) for i in range(len(sc.translates))])
        assert any(r & G.FLIP and kind_of(r) == ffi.VK_KIND_LIST for r in [x for l in sc.lists for x in l] + [c for c, _ in sc.translates]
                   + [c for c, *_ in sc.rotates])
        ok = G.stable(record) & want["hit"]
        hit_kinds = want["object"] >> 28
        winners |= set(hit_kinds[ok].tolist())
        neg = [i for i, (_, r, _) in enumerate(sc.spheres) if r < 0]
        assert np.isin(want["object"][ok], [ffi.make_ref(ffi.VK_KIND_SPHERE, i) for i in neg]).any()
        tm = rays["time"][ok & (hit_kinds == ffi.VK_KIND_MOVING_SPHERE)]
        times |= {name for name, sel in (("below", tm < 0.3), ("inside", (tm > 0.3) & (tm < 0.7)), ("above", tm > 0.7)) if sel.any()}
        assert want["hit"][where["inside_objects"]].all()
    assert axes == {0, 1, 2} and longest >= 7, (axes, longest)               # 6 wrappers and the placing Translate
    assert ("R", ffi.VK_KIND_TRANSLATE) in pairs and ("T", ffi.VK_KIND_ROTATE) in pairs
    assert {ffi.VK_KIND_SPHERE, ffi.VK_KIND_MOVING_SPHERE, ffi.VK_KIND_RECT} <= winners
    assert times == {"below", "inside", "above"}, times


# ================================================================ direct cases: one object, one wrapper, one ray
def _rotate_record(d, child, axis, s, c):
    d.rotates.append(ffi.Rotate(child, axis, float(f32(s)), float(f32(c))))
    return ffi.make_ref(ffi.VK_KIND_ROTATE, len(d.rotates) - 1)


S30, C30 = 0.5, math.sqrt(3.0) / 2.0
# axis, (sin, cos), the sphere's centre C in object space, the ray's direction d, the world centre W, the expected front
ROTATIONS = {
    # RotateY back map (hittable.rs:603-604): x = c x' + s z', z = -s x' + c z'.  C = (2, 0, 0): W = (2c, 0, -2s)
    "y90": (1, (1.0, 0.0), (2, 0, 0), (0, -3, -4), (0.0, 0.0, -2.0), 1),
    "y30": (1, (S30, C30), (2, 0, 0), (0, -3, -4), (2 * C30, 0.0, -1.0), 1),
    # RotateX back map (:692-693): y = c y' - s z', z = s y' + c z'.  C = (0, 2, 0): W = (0, 2c, 2s)
    "x90": (0, (1.0, 0.0), (0, 2, 0), (-3, 0, -4), (0.0, 0.0, 2.0), 1),
    "x30": (0, (S30, C30), (0, 2, 0), (-3, 0, -4), (0.0, 2 * C30, 1.0), 1),
    # RotateZ back map (:781-782): x = c x' - s y', y = s x' + c y'.  C = (2, 0, 0): W = (2c, 2s, 0)
    "z90": (2, (1.0, 0.0), (2, 0, 0), (0, -3, -4), (0.0, 2.0, 0.0), 1),
    "z30": (2, (S30, C30), (2, 0, 0), (0, -3, -4), (2 * C30, 1.0, 0.0), 1),
    # 150 degrees about y, the ray perpendicular to y: the object-space direction d' = (c dx - s dz, 0, s dx + c dz) (:594-595) and the
    # world normal n = -d / 5 give d' . n = -(c (dx^2 + dz^2)) / 5 = -5 c = +4.33 > 0: front = FALSE and the reported normal is
    # +d / 5, pointing AWAY from the ray, although the ray meets the sphere from outside (hittable.rs:618)
    "y150": (1, (0.5, -C30), (2, 0, 0), (-3, 0, -4), (-2 * C30, 0.0, -1.0), 0),
}


def rotation_case(name):
    """A sphere of radius 0.5 at C under one Rotate, met by the ray from O = W - d aimed at its world centre W = back(C), |d| = 5:
    the ray meets it at t = 1 - 0.5 / 5 = 0.9, p = W - 0.1 d, with the outward normal n = -d / 5.  Rotate*::hit then orients n against
    the OBJECT-space direction d' = forward(d): front = (d' . n < 0), normal = n if front else -n.  With n = -d / 5, d' . n = -(d' . d) / 5:
      y (hittable.rs:594-595), d = (0, -3, -4):  d' = (c 0 - s (-4), -3, s 0 + c (-4)) = (4 s, -3, -4 c);  d' . d = 9 + 16 c;
          d' . n = -1.8 - 3.2 c:   y90 (c = 0): -1.8;   y30 (c = 0.8660): -4.571.   Both < 0: front = 1, normal (0, 0.6, 0.8)
      x (:683-684), d = (-3, 0, -4):  d' = (-3, c 0 + s (-4), -s 0 + c (-4)) = (-3, -4 s, -4 c);  d' . d = 9 + 16 c;
          d' . n = -1.8 - 3.2 c:   x90: -1.8;   x30: -4.571.   front = 1, normal (0.6, 0, 0.8)
      z (:772-773), d = (0, -3, -4):  d' = (c 0 + s (-3), -s 0 + c (-3), -4) = (-3 s, -3 c, -4);  d' . d = 9 c + 16;
          d' . n = -3.2 - 1.8 c:   z90: -3.2;   z30: -4.759.   front = 1, normal (0, 0.6, 0.8)
      y150, d = (-3, 0, -4), s = 0.5, c = -0.8660:  d' = (-3 c + 4 s, 0, -3 s - 4 c);  d' . d = 9 c - 12 s + 12 s + 16 c = 25 c;
          d' . n = -5 c = +4.330 > 0: front = 0, normal -n = (-0.6, 0, -0.8)
    p = W - 0.1 d:  y90 (0, 0.3, -1.6), y30 (1.7321, 0.3, -0.6), x90 (0.3, 0, 2.4), x30 (0.3, 1.7321, 1.4), z90 (0, 2.3, 0.4),
    z30 (1.7321, 1.3, 0.4), y150 (-1.4321, 0, -0.6).  A rotation in the wrong sense puts W elsewhere: the ray misses or meets the sphere
    at another p."""
    axis, (s, c), C_, dd, W, front = ROTATIONS[name]
    d = Desc()
    ref = _rotate_record(d, d.sphere(C_, 0.5, d.lambertian(0.5, 0.5, 0.5)), axis, s, c)
    desc = d.finish(d.big_box(ref, ref))
    W, dd = np.array(W, f64), np.array(dd, f64)
    n = -dd / 5.0
    want = dict(t=0.9, p=W - 0.1 * dd, normal=n if front else -n, front=front)
    return d, desc, make_rays([W - dd], [dd]), want


@pytest.mark.parametrize("name", sorted(ROTATIONS))
def test_direct_rotation(name, oracle, emu_rays):
    d, desc, rays, want = rotation_case(name)
    ref, _ = G.reference(G.Scene(desc), rays)
    for who, got in (("oracle", rays_ref.ref_hits(oracle, desc, rays)), ("emulator", emu_rays.trace_rays(desc, rays, 0, 0)[0])):
        check_direct(got[0], want, f"{who} {name}")
    assert ref["hit"][0] and ref["front"][0] == bool(want["front"])
    np.testing.assert_allclose(ref["p"][0], want["p"], atol=1e-6)
    np.testing.assert_allclose(ref["normal"][0], want["normal"], atol=1e-6)


def check_direct(h, want, what):
    assert h["hit"] == 1 and h["front"] == want["front"], f"{what}: {h}"
    np.testing.assert_allclose(h["t"], want["t"], rtol=2e-6, err_msg=what)
    np.testing.assert_allclose(h["p"], want["p"], atol=5e-6, err_msg=what)
    np.testing.assert_allclose(h["normal"], want["normal"], atol=5e-6, err_msg=what)


def translate_cases():
    """A unit sphere at the origin, the ray from its centre along -z: roots -1 and +1, the hit at t = 1 on the BACK face: outward normal
    (0, 0, -1), d . n = +1: front = 0, normal (0, 0, 1) (hittable.rs:85, 23-30).
      bare                front 0, p (0, 0, -1)
      Translate(0, 0, -5) the ray from (0, 0, -5): the child reports the same; Translate::hit calls set_face_normal with the ORIENTED
                          normal (0, 0, 1) (:519): d . n = -1 < 0: front = 1, normal (0, 0, 1), p (0, 0, -6)
      Translate(FlipFace) the child's flip is overwritten: front = 1
      FlipFace(Translate) the flip of the Translate's own answer: front = 0"""
    out = {}
    for name, front, z in (("bare", 0, 0.0), ("translate", 1, -5.0), ("translate_of_flip", 1, -5.0), ("flip_of_translate", 0, -5.0)):
        d = Desc()
        ref = d.sphere((0, 0, 0), 1.0, d.lambertian(0.5, 0.5, 0.5))
        if name == "translate_of_flip":
            ref = Desc.flip(ref)
        if name != "bare":
            ref = d.translate(ref, (0, 0, -5))
        if name == "flip_of_translate":
            ref = Desc.flip(ref)
        desc = d.finish(d.big_box(ref, ref))
        out[name] = (d, desc, make_rays([[0, 0, z]], [[0, 0, -1]]), dict(t=1.0, p=[0, 0, z - 1.0], normal=[0, 0, 1], front=front))
    return out


@pytest.mark.parametrize("name", ["bare", "translate", "translate_of_flip", "flip_of_translate"])
def test_direct_translate_back_face(name, oracle, emu_rays):
    d, desc, rays, want = translate_cases()[name]
    ref, _ = G.reference(G.Scene(desc), rays)
    assert ref["front"][0] == bool(want["front"]) and ref["t"][0] == 1.0
    for who, got in (("oracle", rays_ref.ref_hits(oracle, desc, rays)), ("emulator", emu_rays.trace_rays(desc, rays, 0, 0)[0])):
        check_direct(got[0], want, f"{who} {name}")


def moving_sphere_case():
    """MovingSphere::center (hittable.rs:147-150) does not clamp: centres (0, 0, -5) at time0 = 1 and (2, 0, -5) at time1 = 2 put the
    sphere at x = -2 at time 0, x = 1 at time 1.5 and x = 4 at time 3.  A ray down -z from (x, 0, 0) meets radius 0.5 at t = 4.5."""
    d = Desc()
    ref = d.moving_sphere((0, 0, -5), (2, 0, -5), 1.0, 2.0, 0.5, d.lambertian(0.5, 0.5, 0.5))
    desc = d.finish(d.big_box(ref, ref))
    rays = make_rays([[-2, 0, 0], [1, 0, 0], [4, 0, 0], [0, 0, 0], [2, 0, 0]], [[0, 0, -1]] * 5, time=f32([0.0, 1.5, 3.0, 0.0, 3.0]))
    return d, desc, rays


def check_moving_sphere(got, who):
    assert list(got["hit"]) == [1, 1, 1, 0, 0], who
    np.testing.assert_allclose(got["t"][:3], 4.5, rtol=1e-6, err_msg=who)
    np.testing.assert_allclose(got["p"][:3], [[-2, 0, -4.5], [1, 0, -4.5], [4, 0, -4.5]], atol=5e-6, err_msg=who)


def test_direct_moving_sphere_outside_its_shutter(oracle, emu_rays):
    d, desc, rays = moving_sphere_case()
    ref64, _ = G.reference(G.Scene(desc), rays)
    assert list(ref64["hit"].astype(int)) == [1, 1, 1, 0, 0]
    for who, got in (("oracle", rays_ref.ref_hits(oracle, desc, rays)), ("emulator", emu_rays.trace_rays(desc, rays, 0, 0)[0])):
        check_moving_sphere(got, who)


def rect_bounds_case():
    """Rect::hit (hittable.rs:232, 237): t == tmax and a point ON the edge are hits (u = 1 at a = c1, v = 1 at b = d1); one ulp below
    t, tmax cuts the rect off"""
    d = Desc()
    r = d.xy_rect(-1, 1, -2, 2, -4.0, d.lambertian(0.5, 0.5, 0.5))
    desc = d.finish(d.big_box(r, r))
    rays = make_rays([[1, 0, 0], [-1, 2, 0], [0, 0, 0], [0, 0, 0]], [[0, 0, -1]] * 4, tmax=f32([np.inf, np.inf, 4.0, np.nextafter(f32(4), f32(0))]))
    return d, desc, rays


def check_rect_bounds(got, who):
    assert list(got["hit"]) == [1, 1, 1, 0], who
    assert list(got["u"][:2]) == [1.0, 0.0] and list(got["v"][:2]) == [0.5, 1.0], who
    assert list(got["t"][:3]) == [4.0, 4.0, 4.0], who


def test_direct_rect_bounds_are_inclusive(oracle, emu_rays):
    d, desc, rays = rect_bounds_case()
    ref64, _ = G.reference(G.Scene(desc), rays)
    assert list(ref64["hit"].astype(int)) == [1, 1, 1, 0]
    np.testing.assert_allclose(np.stack([ref64["u"][:2], ref64["v"][:2]]), [[1.0, 0.0], [0.5, 1.0]])
    for who, got in (("oracle", rays_ref.ref_hits(oracle, desc, rays)), ("emulator", emu_rays.trace_rays(desc, rays, 0, 0)[0])):
        check_rect_bounds(got, who)


# ================================================================ media
MEDIA_N = 20000


def media_cases():
    """name -> (builder, origin, direction, time, tmax).  Each is ONE ray traced at MEDIA_N indices: the index is the stream.
    The world holds the medium and, far off the ray, a small sphere (a BVH needs two children; the medium twice would draw twice)."""
    def build(boundary, density):
        def f():
            d = Desc()
            iso = d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(0.8, 0.8, 0.8))
            med = d.medium(boundary(d, d.lambertian(1, 1, 1)), density, iso)
            return d, d.finish(d.big_box(med, d.sphere((500, 500, 500), 0.1, d.lambertian(0.5, 0.5, 0.5))))
        return f
    sphere = lambda d, m: d.sphere((0, 0, -5), 2.0, m)
    boxy = lambda d, m: d.boxy((-1, -1, -7), (1, 1, -3), m)
    moving = lambda d, m: d.moving_sphere((0, 0, -5), (0, 3, -5), 0.0, 1.0, 2.0, m)
    inf = np.inf
    return {
        "sphere-through-|d|=3": (build(sphere, 0.4), (0.5, 0, 0), (0, 0, -3), 0.0, inf),
        "sphere-from-inside-|d|=0.5": (build(sphere, 0.7), (0.3, 0.2, -4.5), (0.3, 0.1, -0.3872983), 0.0, inf),
        "sphere-tmax-cuts-|d|=2": (build(sphere, 0.5), (0, 0.5, 0), (0, 0, -2), 0.0, 2.6),
        "boxy-oblique-|d|=0.25": (build(boxy, 0.6), (0.2, 0.1, 0), (0.02, 0.03, -0.2473863), 0.0, inf),
        "boxy-from-inside": (build(boxy, 0.3), (0, 0, -5), (1.0, 0.5, -3.0), 0.0, inf),
        "moving-sphere-at-0.5-|d|=1.5": (build(moving, 0.5), (0, 1.0, 0), (0, 0, -1.5), 0.5, inf),
    }


def media_rays(name):
    build, o, dd, time, tmax = media_cases()[name]
    d, desc = build()
    return d, desc, make_rays(np.tile(f32(o), (MEDIA_N, 1)), np.tile(f32(dd), (MEDIA_N, 1)), time, tmax)


def check_medium(desc, rays, hits, what):
    """the scatter frequency within 4 binomial standard errors of 1 - exp(-density length |d|-scaled); the mean and the second moment of
    the scatter distance within 4 SE of the truncated exponential's; the power control — the chord in units of t, not of t |d| — rejected
    by the same data at |z| > 4.  Returns the z scores."""
    sc = G.Scene(desc)
    o, dd, time, tmax = G.rays_f64(rays[:1])
    valid, t_in, t_out, length = G.medium_segment(sc, 0, o, dd, time, G.TMIN, tmax)
    assert valid[0]
    rho, L, speed = G.medium_density(sc, 0), float(length[0]), float(np.linalg.norm(dd[0]))
    n, scattered = len(rays), hits["hit"] == 1
    assert (hits["medium"][scattered] == 1).all() and (hits["object"][scattered] == ffi.make_ref(ffi.VK_KIND_MEDIUM, 0)).all(), what
    assert (hits["material"][scattered] == sc.media[0][2]).all(), what
    z_of = lambda P: (scattered.sum() - n * P) / math.sqrt(n * P * (1 - P))
    P = float(G.scatter_probability(rho, L))
    z = {"P": z_of(P), "control": z_of(float(G.scatter_probability(rho, L / speed)))}
    assert 0.05 < P < 0.95, f"{what}: P = {P} tests little"
    assert abs(z["P"]) <= 4.0, f"{what}: {scattered.sum()} of {n} scatter, expected {n * P:.1f}: z = {z['P']:.2f}"
    assert abs(z["control"]) > 4.0, f"{what}: the power control is not rejected, z = {z['control']:.2f}"
    s = (hits["t"][scattered].astype(f64) - float(t_in[0])) * speed
    assert (s >= -1e-5 * max(1.0, L)).all() and (s <= L * (1 + 1e-5)).all(), what
    for k, want in zip((1, 2), G.scatter_moments(rho, L)):
        x = s ** k
        z[f"s^{k}"] = (x.mean() - want) / (x.std(ddof=1) / math.sqrt(len(x)))
        assert abs(z[f"s^{k}"]) <= 4.0, f"{what}: mean of s^{k} {x.mean():.6g}, expected {want:.6g}: z = {z[f's^{k}']:.2f}"
    # p = o + t d (hittable.rs:482) and the arbitrary normal and front of a medium record (:483-487)
    np.testing.assert_allclose(hits["p"][scattered], o[0] + hits["t"][scattered, None].astype(f64) * dd[0], rtol=0, atol=1e-5 * (1 + np.abs(o[0]).max() + L))
    assert (hits["normal"][scattered] == f32([1, 0, 0])).all() and (hits["front"][scattered] == 1).all(), what
    return z


@pytest.mark.parametrize("name", sorted(media_cases()))
def test_medium(name, oracle, emu_rays):
    d, desc, rays = media_rays(name)
    for who, hits in (("oracle", rays_ref.ref_hits(oracle, desc, rays, SEED, 0)), ("emulator", emu_rays.trace_rays(desc, rays, SEED, 0)[0])):
        z = check_medium(desc, rays, hits, f"{who} {name}")
        print(f"\n   {who} {name}: z " + ", ".join(f"{k} {v:.2f}" for k, v in z.items()))


# ================================================================ textures
N_TEX = 4096
IMAGE_SIZES = ((1, 1), (1, 7), (5, 3), (32, 16))          # width x height


def texture_scene():
    """(owner, desc, name -> texture index): a checker over two solids, four images, two noises"""
    d = Desc()
    rng = np.random.default_rng(77)
    tex = {"checker": d.checker(d.solid(0.1, 0.2, 0.3), d.solid(0.9, 0.8, 0.7))}
    for w, h in IMAGE_SIZES:
        tex[f"image-{w}x{h}"] = d.image(rng.integers(0, 256, (h, w, 3)))
    tex["checker-of-images"] = d.checker(tex["image-5x3"], tex["image-32x16"])
    tex["noise-0.1"], tex["noise-4"] = d.noise(0.1, seed=1), d.noise(4.0, seed=2)
    m = d.lambertian(0.5, 0.5, 0.5)
    s = d.sphere((0, 0, 0), 1.0, m)
    return d, d.finish(d.big_box(s, s)), tex


def texture_points(name):
    """(u, v, p) f32: u and v over [-0.25, 1.25] (the clamp) with the corners and borders themselves; p in all eight octants"""
    rng = np.random.default_rng(sum(map(ord, name)))
    u, v = rng.uniform(-0.25, 1.25, N_TEX).astype(f32), rng.uniform(-0.25, 1.25, N_TEX).astype(f32)
    u[:8], v[:8] = f32([0, 1, 0, 1, 0.5, 1, 0, 0.999999]), f32([0, 0, 1, 1, 1, 0.5, 0.5, 0.000001])
    p = (rng.uniform(0.05, 9.0, (N_TEX, 3)) * rng.choice([-1.0, 1.0], (N_TEX, 3))).astype(f32)
    octants = {tuple(r) for r in (p > 0).tolist()}
    assert len(octants) == 8
    return u, v, p


TEXTURES = ["checker", "checker-of-images", "noise-0.1", "noise-4"] + [f"image-{w}x{h}" for w, h in IMAGE_SIZES]


def texture_deviation(got, sc, index, u, v, p, what):
    """largest |got - f64| over the points whose discrete decisions are stable; at most 1 % are not"""
    want, margin = G.texture_value(sc, index, u, v, p)
    ok = margin >= 1.0
    assert ok.mean() >= 1.0 - G.MAX_EXCLUDED, f"{what}: {1 - ok.mean():.4f} of the points sit on a texel border or a checker's zero"
    return float(np.abs(got.astype(f64) - want)[ok].max())


@pytest.mark.parametrize("name", TEXTURES)
def test_texture(name, oracle):
    d, desc, tex = texture_scene()
    u, v, p = texture_points(name)
    dev = texture_deviation(oracle.texture_values(desc, tex[name], u, v, p), G.Scene(desc), tex[name], u, v, p, name)
    print(f"\n   {name}: oracle - f64 {dev:.3g}")
    assert dev <= G.BOUND["noise" if name.startswith("noise") else "albedo"], f"{name}: {dev}"


def test_checker_at_an_exact_zero_is_even(oracle):
    """Checker::value (material.rs:252-257) takes `odd` where the product of sines is < 0: at a point with a coordinate exactly 0 the
    product is +-0, which is not < 0, so the value is `even` whatever the other two sines' signs"""
    d, desc, tex = texture_scene()
    p = f32([[0, 0.1, 0.1], [0, 0.4, 0.1], [0.1, 0, 0.4], [0.4, 0.1, 0], [0, 0, 0], [0.4, 0.4, 0.0]])       # sin(4) < 0 < sin(1)
    want, _ = G.texture_value(G.Scene(desc), tex["checker"], np.zeros(6), np.zeros(6), p)
    np.testing.assert_allclose(want, np.tile([0.9, 0.8, 0.7], (6, 1)), atol=1e-7)
    np.testing.assert_allclose(oracle.texture_values(desc, tex["checker"], np.zeros(6), np.zeros(6), p), want, atol=1e-7)


def checker_zero_case():
    """Rays down -z from (x, y, 3) onto an xy_rect at z = 0 that carries the checker: t = (0 - 3) / -1 = 3 and p.z = 3 + 3 * -1 = 0
    EXACTLY (hittable.rs:231, main.rs:51-53), so the product of sines is +-0 and the value is `even`, (0.9, 0.8, 0.7), at every point —
    also where sin(10 x) sin(10 y) < 0 ((0.4, 0.1): sin 4 < 0 < sin 1).  One bounce of the scatter integrator on such a hit multiplies the
    throughput by the Lambertian's albedo (material.rs:85-90, main.rs:135): the state's thr IS the texture value.  This is the only
    route on which the emulator and the device evaluate a Checker at a sine that is exactly 0."""
    d = Desc()
    chk = d.checker(d.solid(0.1, 0.2, 0.3), d.solid(0.9, 0.8, 0.7))
    r = d.xy_rect(-2, 2, -2, 2, 0.0, d.mat(ffi.VK_MAT_LAMBERTIAN, chk))
    desc = d.finish(d.big_box(r, r))
    xy = [[0.1, 0.1], [0.4, 0.1], [0.1, 0.4], [0.4, 0.4], [-0.4, 0.1], [0.7, -0.1]]
    return d, desc, make_rays([[x, y, 3.0] for x, y in xy], [[0, 0, -1]] * len(xy))


def check_checker_zero(hits, shaded, who):
    assert (hits["hit"] == 1).all() and (hits["p"][:, 2] == 0.0).all(), who
    assert (shaded["status"] == ffi.VK_SHADE_SCATTERED).all(), who
    np.testing.assert_array_equal(shaded["state"]["thr"], np.tile(f32([0.9, 0.8, 0.7]), (len(hits), 1)), err_msg=who)


def test_checker_at_an_exact_zero_through_a_bounce(emu_rays, built):
    import emu_shade_ffi
    from vecchio_amd.scene import make_path_states
    d, desc, rays = checker_zero_case()
    hits = emu_rays.trace_rays(desc, rays, 0, 0)[0]
    shaded = emu_shade_ffi.shade_hits(desc, rays, hits, make_path_states(len(rays)), integrator=ffi.VK_INTEGRATOR_SCATTER)
    check_checker_zero(hits, shaded, "emulator")


def test_image_texel_by_hand():
    """ImageTexture::value (material.rs:283-303) on a 5 x 3 image: u = 0.5 is column (0.5 * 5) as usize = 2; v = 0.9 is row
    ((1 - 0.9) * 3) as usize = 0, the TOP row of the buffer; v = 0.1 is row 2, the bottom one; u = 1 and v = 0 clamp to column 4, row 2"""
    d = Desc()
    img = np.arange(45, dtype=np.uint8).reshape(3, 5, 3)
    t = d.image(img)
    s = d.sphere((0, 0, 0), 1.0, d.lambertian(0.5, 0.5, 0.5))
    sc = G.Scene(d.finish(d.big_box(s, s)))
    rgb, _ = G.texture_value(sc, t, [0.5, 0.5, 1.0], [0.9, 0.1, 0.0], np.zeros((3, 3)))
    np.testing.assert_allclose(rgb * 255.0, [img[0, 2], img[2, 2], img[2, 4]], atol=1e-12)


def test_perlin_cast_of_a_negative_floor_by_hand():
    """Perlin::noise (material.rs:399-401): floor(-0.25) = -1 cast to usize saturates to 0, so the lattice cell of x = -0.25 is cell 0
    with u = 0.75 — the same value as x = +0.75 in cell 0, and NOT the value of a lattice that continues below zero"""
    d = Desc()
    t = d.noise(1.0, seed=3)
    s = d.sphere((0, 0, 0), 1.0, d.lambertian(0.5, 0.5, 0.5))
    sc = G.Scene(d.finish(d.big_box(s, s)))
    pl = sc.perlins[0]
    a = G.perlin_noise(pl, np.array([[-0.25, 0.4, 0.6], [-3.25, 0.4, 0.6]]))
    b = G.perlin_noise(pl, np.array([[0.75, 0.4, 0.6]]))
    assert a[0] == b[0] == a[1]


def sphere_uv_rays():
    """rays aimed at the centre of a unit sphere from all round it, a ring of them across the seam (x < 0, z about 0) and some near both
    poles: 4096"""
    rng = np.random.default_rng(5)
    n = rng.normal(size=(N_TEX, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    k = 256
    y = rng.uniform(-0.9, 0.9, k)
    z = rng.uniform(-0.01, 0.01, k)
    n[:k] = np.stack([-np.sqrt(1 - y * y - z * z), y, z], 1)
    n[k:k + 64, 1] = rng.choice([-1.0, 1.0], 64) * 5.0
    n[k:k + 64] /= np.linalg.norm(n[k:k + 64], axis=1, keepdims=True)
    return make_rays((3.0 * n).astype(f32), (-n * rng.uniform(0.5, 2.0, (N_TEX, 1))).astype(f32))


def test_spherical_uv_over_the_whole_sphere(oracle, emu_rays):
    d = Desc()
    s = d.sphere((0, 0, 0), 1.0, d.lambertian(0.5, 0.5, 0.5))
    desc = d.finish(d.big_box(s, s))
    rays = sphere_uv_rays()
    want, record = G.reference(G.Scene(desc), rays)
    assert want["hit"].all() and (record["seam"] < G.SEAM_MIN).sum() > 10
    # u runs DOWN with atan2(z, x) (the `1 -` of hittable.rs:58): at (x, z) = (1, 0) u = 0.5, at (0, 1) 0.25, at (0, -1) 0.75; v = 0 at y = -1
    uu, vv = G.spherical(np.array([[1.0, 0, 0], [0, 0, 1.0], [0, 0, -1.0], [0, -1.0, 0]]))
    np.testing.assert_allclose(uu[:3], [0.5, 0.25, 0.75])
    assert vv[3] == 0.0
    for who, got in (("oracle", rays_ref.ref_hits(oracle, desc, rays)), ("emulator", emu_rays.trace_rays(desc, rays, 0, 0)[0])):
        # (the rays near the poles are excluded from u and v by the record, and counted: under the cap)
        worst = G.compare_hits(got, want, record, rays, f"{who} sphere uv")
        print(f"\n   sphere uv, {who} - f64: " + ", ".join(f"{k} {worst[k]:.3g}" for k in ("t", "p", "normal", "uv", "excluded")))
        G.assert_within(worst, f"{who} sphere uv")


# ================================================================ camera
CAMERAS = [dict(lookfrom=(3, 2, 5), lookat=(0.5, 0.2, -1), vup=(0.2, 1.0, 0.1), vfov=vfov, aspect=aspect, aperture=aperture, focus=4.5,
                t0=0.25, t1=1.75) for vfov in (20.0, 90.0) for aspect in (1.0, 16.0 / 9.0, 0.5) for aperture in (0.0, 0.3)]
FRAMES = ((2, 2), (2, 3), (3, 2), (8, 8), (21, 13))  # width x height.  A frame 1 wide or 1 high has width - 1 = 0 or height - 1 = 0: s = x / 0
#                                                     (main.rs:187) is +inf or a NaN.  The library refuses such a frame (VK_ERR_BAD_ARG,
#                                                     "width/height must be >= 2"), 1 x 2 and 2 x 1 as well as 1 x 1:
#                                                     test_a_frame_one_pixel_wide_or_high_is_refused.  Left as it is.
CAM_SEED, CAM_SPP = 11, 2


def camera_id(c):
    return f"vfov{c['vfov']:g}-aspect{c['aspect']:.2f}-aperture{c['aperture']:g}"


def check_camera_rays(c, width, height, o, dd, time, xi, what, x0=0, y0=0):
    """o, dd, time: (h, w, n, ...) of an f32 evaluation of the window of w x h pixels at (x0, y0) of a width x height frame; xi: the
    same window of geometry_ref.stream_draws.  Returns the worst deviation of origin + direction from the f64 focus point and of the
    origin from the lens plane, relative to the focus distance."""
    cam = G.camera_new(c["lookfrom"], c["lookat"], c["vup"], c["vfov"], c["aspect"], c["aperture"], c["focus"], c["t0"], c["t1"])
    y, x = np.mgrid[y0:y0 + o.shape[0], x0:x0 + o.shape[1]]
    s, t = G.pixel_st(xi, x[..., None], y[..., None], width, height)
    want = G.focus_point(cam, s, t)
    o, dd = o.astype(f64), dd.astype(f64)
    dev = float(np.abs(o + dd - want).max()) / c["focus"]
    a, b, w = G.lens_coordinates(cam, o)
    dev = max(dev, float(np.abs(w).max()) / c["focus"])
    r = np.sqrt(a * a + b * b)
    if c["aperture"] == 0.0:
        assert (o == f32(c["lookfrom"]).astype(f64)).all(), f"{what}: aperture 0 moves the origin"
    else:
        assert (r < cam["lens_radius"] * (1 + 1e-6)).all(), f"{what}: an origin outside the lens disc"
        if r.size >= 64:                                   # uniform over the disc: mean r^2 = R^2 / 2, a fifth of the origins beyond 0.9 R
            assert (r > 0.9 * cam["lens_radius"]).mean() > 0.05 and abs((r * r).mean() / cam["lens_radius"] ** 2 - 0.5) < 0.15, what
    assert ((time >= f32(c["t0"])) & (time < f32(c["t1"]))).all(), f"{what}: a time outside [time0, time1)"
    if time.size >= 64:
        assert time.min() < c["t0"] + 0.2 * (c["t1"] - c["t0"]) and time.max() > c["t1"] - 0.2 * (c["t1"] - c["t0"]), what
    return dev


@pytest.mark.parametrize("c", CAMERAS, ids=camera_id)
def test_camera(c, oracle, built):
    import emu_film_ffi
    d = Desc()
    s = d.sphere((0, 0, -100), 1.0, d.lambertian(0.5, 0.5, 0.5))
    desc = d.finish(d.big_box(s, s))
    cam = camera(c["lookfrom"], c["lookat"], c["vfov"], c["aspect"], c["aperture"], c["focus"], c["t0"], c["t1"], c["vup"])
    # the host mirror's Camera::new against main.rs:71-109
    want = G.camera_new(c["lookfrom"], c["lookat"], c["vup"], c["vfov"], c["aspect"], c["aperture"], c["focus"], c["t0"], c["t1"])
    worst = 0.0
    for k in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w"):
        worst = max(worst, float(np.abs(np.array(list(getattr(cam, k)), f64) - want[k]).max()) / (c["focus"] if k in ("lower_left_corner", "horizontal", "vertical") else 1.0))
    assert worst <= G.BOUND["camera"], f"vkh_camera_new deviates by {worst}"
    devs = [worst]
    assert cam.lens_radius == f32(c["aperture"] / 2) and cam.time0 == f32(c["t0"]) and cam.time1 == f32(c["t1"])
    for width, height in FRAMES:
        p = params(width, height, CAM_SPP, seed=CAM_SEED, integrator=ffi.VK_INTEGRATOR_SCATTER)
        xi = G.stream_draws(oracle.draws, CAM_SEED, width, height, CAM_SPP)
        fh = oracle.first_hits(desc, cam, p, 0, CAM_SPP)
        dev = check_camera_rays(c, width, height, fh["origin"], fh["direction"], fh["time"], xi, f"oracle {width}x{height}")
        rays, states = emu_film_ffi.emit(cam, p, 0, 0, width, height, 0, CAM_SPP)
        shape = (height, width, CAM_SPP)
        dev_e = check_camera_rays(c, width, height, rays["origin"].reshape(shape + (3,)), rays["direction"].reshape(shape + (3,)),
                                  rays["time"].reshape(shape), xi, f"emulator emit {width}x{height}")
        # id ((y - y0) * w + (x - x0)) * n_samples + k is sample k of pixel (x, y)
        y, x, k = np.mgrid[0:height, 0:width, 0:CAM_SPP]
        assert (states["pixel"].reshape(shape) == y * width + x).all() and (states["sample"].reshape(shape) == k).all()
        devs.append(max(dev, dev_e))
        assert max(dev, dev_e) <= G.BOUND["camera"], (width, height, dev, dev_e)
    print(f"\n   {camera_id(c)}: vkh_camera_new - f64 {devs[0]:.3g}; oracle / emulator rays - f64 {max(devs[1:]):.3g} of the focus distance")


def test_a_frame_one_pixel_wide_or_high_is_refused(oracle, built):
    d = Desc()
    s = d.sphere((0, 0, -100), 1.0, d.lambertian(0.5, 0.5, 0.5))
    desc = d.finish(d.big_box(s, s))
    cam = camera((0, 0, 0), (0, 0, -1))
    for width, height in ((1, 1), (1, 2), (2, 1)):
        with pytest.raises(RuntimeError, match="must be >= 2"):
            oracle.first_hits(desc, cam, params(width, height, 1), 0, 1)


# ================================================================ first-hit buffers
def carrier_scene():
    """Lambertian carriers of an image, a checker of image and solid, and two noise textures: three spheres, a floor rect and a Boxy under
    a rotation and a translation, seen from a pinhole camera"""
    d = Desc()
    rng = np.random.default_rng(3)
    img = d.image(rng.integers(0, 256, (16, 32, 3)))
    chk = d.checker(d.solid(0.125, 0.25, 0.5), img)
    lam = lambda t: d.mat(ffi.VK_MAT_LAMBERTIAN, t)
    objs = [d.sphere((-1.6, 0.1, 0.3), 1.0, lam(img)), d.sphere((1.5, 0.4, -0.2), 1.2, lam(chk)), d.sphere((0.1, 2.2, -1.0), 0.8, lam(d.noise(4.0, seed=5))),
            d.xz_rect(-6, 6, -6, 6, -1.0, lam(d.noise(0.1, seed=6))),
            d.translate(d.rotate(d.boxy((-0.5, -0.5, -0.5), (0.5, 0.7, 0.9), lam(chk)), 1, 35.0), (0.2, -0.3, 2.0))]
    world = objs[0]
    for o in objs[1:]:
        world = d.big_box(world, o)
    return d, d.finish(world)


AOV_W, AOV_H, AOV_SEED = 32, 24, 5
AOV_CAM = dict(lookfrom=(0.5, 3.0, 8.0), lookat=(0, 0.3, 0), vup=(0, 1, 0), vfov=40.0, aspect=AOV_W / AOV_H, aperture=0.0, focus=7.0, t0=0.0, t1=1.0)


def aov_reference(oracle, desc):
    """per pixel: the f64 hit of the f64 camera ray of sample 0 (aperture 0: the ray is lookfrom -> the focus point of the stream's two
    draws), its albedo, and which pixels are stable (the hit's record, the texture's margins)"""
    c = AOV_CAM
    cam = G.camera_new(c["lookfrom"], c["lookat"], c["vup"], c["vfov"], c["aspect"], c["aperture"], c["focus"], c["t0"], c["t1"])
    xi = G.stream_draws(oracle.draws, AOV_SEED, AOV_W, AOV_H, 1)
    y, x = np.mgrid[0:AOV_H, 0:AOV_W]
    s, t = G.pixel_st(xi[:, :, 0], x, y, AOV_W, AOV_H)
    o = np.broadcast_to(cam["origin"], (AOV_H * AOV_W, 3))
    dd = (G.focus_point(cam, s, t) - cam["origin"]).reshape(-1, 3)
    sc = G.Scene(desc)
    hit, record = G.closest_hit(sc, o, dd)
    albedo, margin = G.albedo_of(sc, hit)
    ok = G.uv_stable(record) & (margin >= 1.0) & (record["seam"] >= G.SEAM_MIN)
    depth = np.where(hit["hit"], hit["t"] * np.linalg.norm(dd, axis=1), np.inf)
    shape = (AOV_H, AOV_W)
    return dict(hit=hit["hit"].reshape(shape), albedo=albedo.reshape(shape + (3,)), normal=hit["normal"].reshape(shape + (3,)),
                depth=depth.reshape(shape), ok=ok.reshape(shape), stable=G.stable(record).reshape(shape))


def check_aov(got, want, what):
    """got: albedo, normal, depth, coverage of a 1 spp first-hit buffer.  Coverage exact on the stable pixels; albedo on the pixels whose
    texture decisions are stable too.  Returns the worst deviations."""
    st, ok = want["stable"], want["ok"]
    assert 1.0 - st.mean() <= G.MAX_EXCLUDED, f"{what}: {1 - st.mean():.4f} of the pixels' rays are unstable"
    assert 1.0 - ok.mean() <= G.MAX_EXCLUDED, f"{what}: {1 - ok.mean():.4f} of the pixels are unstable (ray, pole, seam, texel border or checker zero)"
    assert ((got["coverage"] == 1.0) == want["hit"])[st].all(), f"{what}: coverage"
    h = st & want["hit"]
    assert h.mean() > 0.5
    dev = dict(normal=float(np.abs(got["normal"].astype(f64) - want["normal"])[h].max()),
               t=float(np.abs(got["depth"].astype(f64)[h] / want["depth"][h] - 1.0).max()))
    h = ok & want["hit"]
    dev["albedo"] = float(np.abs(got["albedo"].astype(f64) - want["albedo"])[h].max())
    return dev


def test_first_hit_buffers(oracle, emu):
    d, desc = carrier_scene()
    c = AOV_CAM
    cam = camera(c["lookfrom"], c["lookat"], c["vfov"], c["aspect"], c["aperture"], c["focus"], c["t0"], c["t1"], c["vup"])
    p = params(AOV_W, AOV_H, 1, seed=AOV_SEED, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SOLID)
    want = aov_reference(oracle, desc)
    import aov_ref
    r = aov_ref.ref_a(oracle, desc, cam, p, [0])                 # (oracle.first_hits and oracle.texture_values, put together)
    o = {k: r[k][0] for k in ("albedo", "normal", "depth", "coverage")}
    got, _ = emu.aov_samples(desc, cam, p, 0, 1)
    for who, g in (("oracle", o), ("emulator", got[0])):
        dev = check_aov(g, want, who)
        print(f"\n   first-hit buffers, {who} - f64: " + ", ".join(f"{k} {v:.3g}" for k, v in dev.items()))
        assert dev["albedo"] <= G.BOUND["aov_albedo"] and dev["normal"] <= G.BOUND["normal"] and dev["t"] <= G.BOUND["t"], (who, dev)


# ================================================================ sphere clouds: which sphere does a walk of a rebuilt tree find?
CLOUD_B = (0.5, 0.5, 0.5)
CLOUD_W, CLOUD_H, CLOUD_SPP, CLOUD_SEED = 32, 24, 4, 21


def cloud_colour(k):
    """sphere k's own colour: ((k mod 32) + 1) / 128, (k div 32 + 1) / 128, 1 / 4 — exact in f32, and so is its half"""
    return ((k % 32 + 1) / 128.0, (k // 32 + 1) / 128.0, 0.25)


def cloud_decode(samples, scale):
    """per sample: the sphere its colour names, -1 for the background B, -2 for black"""
    x = np.asarray(samples, f64)[:, :3]
    k = np.full(len(x), -3)
    k[(x == np.asarray(CLOUD_B)).all(1)] = -1
    k[(x == 0).all(1)] = -2
    named = x[:, 2] == 0.25 * scale
    j = x[named, :2] * (128.0 / scale)
    assert (j == np.round(j)).all() and (j >= 1).all()
    k[named] = (j[:, 0] - 1) + 32 * (j[:, 1] - 1)
    assert (k != -3).all(), "a sample that is neither a sphere's colour times B, nor B, nor 0"
    return k


def _tree_of_spheres(d, objs):
    """a BVH over (ref, lo, hi): halves along the longest axis of the centres, a node's box the union of its children's"""
    if len(objs) == 1:
        return objs[0]
    ctr = np.array([(o[1] + o[2]) / 2 for o in objs])
    axis = int(np.argmax(ctr.max(0) - ctr.min(0)))
    objs = sorted(objs, key=lambda o: (o[1][axis] + o[2][axis]))
    left, right = _tree_of_spheres(d, objs[:len(objs) // 2]), _tree_of_spheres(d, objs[len(objs) // 2:])
    lo, hi = np.minimum(left[1], right[1]), np.maximum(left[2], right[2])
    return d.bvh_node(left[0], right[0], tuple(float(x) for x in lo), tuple(float(x) for x in hi)), lo, hi


def cloud(name):
    """(owner, desc, cam, p, scale): `layer` — a ground sphere of radius 1000 beside 25 of radius 0.35 and 3 of radius 1 (29); `shared` —
    40 spheres of radius 0.9375 on a flat 5 x 8 lattice of spacing 2, so that every coordinate is shared by many; `inside` — 48 small spheres in front of a camera
    that sits inside a 49th of radius 6; `grid` — 81 spheres of radius 0.4 in a layer on a ground sphere, and 2 of radius 1.1 (84: the grid
    form of exact re-treeing takes no world of fewer than 72 spheres, vk_linearize.cpp rt_build_grid).  layer, shared and grid: Lambertian colours under the solid background B at max_depth 2, so a sample is
    colour_k * B where the scattered ray leaves, 0 where it meets something, B where the primary ray misses.  inside: nothing leaves the
    big sphere, so its spheres are DiffuseLights at max_depth 1: a sample is colour_k on a front face and 0 on the big sphere's inside."""
    d = Desc()
    rng = np.random.default_rng(sum(map(ord, name)))
    spheres = []
    if name == "layer":
        spheres.append(((0.0, -1000.0, 0.0), 1000.0))
        for i in range(5):
            for j in range(5):
                spheres.append(((2.0 * i - 4.0 + float(rng.uniform(-0.6, 0.6)), 0.35, 2.0 * j - 4.0 + float(rng.uniform(-0.6, 0.6))), 0.35))
        spheres += [((0.0, 1.0, 0.0), 1.0), ((-4.0, 1.0, 0.5), 1.0), ((4.0, 1.0, -0.5), 1.0)]
        cam = camera((13, 4.5, 3), (0, 0.3, 0), vfov=40.0, aspect=CLOUD_W / CLOUD_H, aperture=0.0)
    elif name == "grid":
        spheres.append(((0.0, -1000.0, 0.0), 1000.0))
        for i in range(9):
            for j in range(9):
                spheres.append(((1.0 * i - 4.0 + float(rng.uniform(-0.05, 0.05)), 0.4, 1.0 * j - 4.0 + float(rng.uniform(-0.05, 0.05))), 0.4))
        spheres += [((0.5, 1.1, -5.7), 1.1), ((-0.5, 1.1, 5.7), 1.1)]
        cam = camera((0.3, 14.0, 0.3), (0, 0, 0), vfov=36.0, aspect=CLOUD_W / CLOUD_H, aperture=0.0, vup=(1, 0, 0))
    elif name == "shared":
        spheres = [((2.0 * i, 0.0, 2.0 * k), 0.9375) for i in range(5) for k in range(8)]
        cam = camera((4.5, 19, 7.5), (4, 0, 7), vfov=28.0, aspect=CLOUD_W / CLOUD_H, aperture=0.0, vup=(1, 0, 0))
    else:
        for i in range(8):
            for j in range(6):
                spheres.append(((0.46 * (i - 3.5) + float(rng.uniform(-0.03, 0.03)), 0.46 * (j - 2.5) + float(rng.uniform(-0.03, 0.03)),
                                 -3.0 + float(rng.uniform(-0.4, 0.4))), 0.2))
        spheres.append(((0.3, -0.2, -1.0), 6.0))
        cam = camera((0, 0, 0), (0, 0, -3), vfov=50.0, aspect=CLOUD_W / CLOUD_H, aperture=0.0)
    emissive = name == "inside"
    objs = []
    for k, (c, r) in enumerate(spheres):
        m = d.light(*cloud_colour(k)) if emissive else d.lambertian(*cloud_colour(k))
        # the box of a sphere as the reference makes it (hittable.rs:97-102): centre -+ radius in f32, from the f32 record — a box
        # rounded from f64 can cut a sphere by an ulp, and a tree whose boxes do not hold their spheres is walked as handed over
        c = np.array(c, f32)
        objs.append((d.sphere(tuple(float(x) for x in c), r, m), c - f32(r), c + f32(r)))
    desc = d.finish(_tree_of_spheres(d, objs)[0], [])
    p = params(CLOUD_W, CLOUD_H, CLOUD_SPP, max_depth=1 if emissive else 2, seed=CLOUD_SEED, integrator=ffi.VK_INTEGRATOR_SCATTER,
               background=ffi.VK_BACKGROUND_SOLID, bg=CLOUD_B)
    return d, desc, cam, p, (1.0 if emissive else 0.5)


CLOUDS = ("layer", "shared", "inside", "grid")
_cloud_cache = {}


def cloud_winners(name, oracle):
    """(winner, stable) per sample in render_samples' order [pixel * spp + s]: the sphere the f64 closest hit of the sample's f64 camera
    ray names (-1: none), and whether that ray is stable"""
    if name not in _cloud_cache:
        d, desc, cam, p, scale = cloud(name)
        xi = G.stream_draws(oracle.draws, CLOUD_SEED, CLOUD_W, CLOUD_H, CLOUD_SPP)
        y, x = np.mgrid[0:CLOUD_H, 0:CLOUD_W]
        s, t = G.pixel_st(xi, x[..., None], y[..., None], CLOUD_W, CLOUD_H)
        c64 = {k: np.array(list(getattr(cam, k)), f64) for k in ("origin", "lower_left_corner", "horizontal", "vertical")}
        dd = (G.focus_point(c64, s, t) - c64["origin"]).reshape(-1, 3)
        hit, record = G.closest_hit(G.Scene(desc), np.broadcast_to(c64["origin"], dd.shape), dd)
        winner = np.where(hit["hit"], (hit["object"] & G.INDEX_MASK).astype(np.int64), -1)
        front = hit["front"]
        _cloud_cache[name] = (winner, G.stable(record), front)
    return _cloud_cache[name]


def check_cloud(name, samples, oracle, what, conditions=True):
    """every sample that names a sphere names the f64 winner of its primary ray; B only where the f64 ray misses; and (the conditions)
    at least half of the samples name a sphere, every sphere that wins a stable ray is named at least once"""
    d, desc, cam, p, scale = cloud(name)
    winner, ok, front = cloud_winners(name, oracle)
    assert 1.0 - ok.mean() <= G.MAX_EXCLUDED, f"{what}: {1 - ok.mean():.4f} unstable"
    k = cloud_decode(samples, scale)
    named = k >= 0
    bad = np.flatnonzero(ok & named & (k != winner))
    assert len(bad) == 0, f"{what}: {len(bad)} samples name another sphere than the f64 winner; first {bad[0]}: {k[bad[0]]} for {winner[bad[0]]}"
    bad = np.flatnonzero(ok & ((k == -1) != (winner == -1)))
    assert len(bad) == 0, f"{what}: {len(bad)} samples disagree on the miss; first {bad[0]}: {k[bad[0]]} for {winner[bad[0]]}"
    if scale == 1.0:                      # emitters: black exactly on the back faces
        bad = np.flatnonzero(ok & (winner >= 0) & ((k == -2) != ~front))
        assert len(bad) == 0, f"{what}: {len(bad)} samples disagree on the face; first {bad[0]}"
    if conditions:
        in_view = set(winner[ok & (winner >= 0) & (front | (scale != 1.0))].tolist())
        assert named.mean() >= 0.5, f"{what}: only {named.mean():.3f} of the samples name a sphere"
        assert in_view <= set(k[named].tolist()), f"{what}: never named: {sorted(in_view - set(k[named].tolist()))}"
    return float(named.mean()), len(set(k[named].tolist()))


@pytest.mark.parametrize("name", CLOUDS)
def test_cloud_on_the_cpu(name, oracle, emu):
    """the oracle meets both conditions on every cloud, and the emulator's walk of each tree view finds the f64 winners"""
    d, desc, cam, p, scale = cloud(name)
    share, n = check_cloud(name, oracle.render_samples(desc, cam, p)[1], oracle, f"oracle {name}")
    print(f"\n   {name}: {desc.contents.n_spheres} spheres, {n} named, {share:.3f} of the samples name one")
    for flags in (0, ffi.VK_SCENE_REFERENCE_TREE, ffi.VK_SCENE_FAST_ACCEL):
        desc.contents.flags = flags
        check_cloud(name, emu.render_samples(desc, cam, p)[1], oracle, f"emulator {name} flags {flags}")
