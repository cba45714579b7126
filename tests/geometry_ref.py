"""Closed-form geometry below the integrators: first hits, media, textures and camera rays in plain f64 numpy.  TESTS ONLY; shared by
tests/test_geometry.py (oracle, emulator) and tests/test_gpu_geometry.py (the public ABI on the device).

Everything here is written from the reference's own lines (hittable.rs, accel.rs, material.rs, main.rs), cited beside each function, and
shares nothing with the library's restatement of them: no import of the oracle, of an emulator or of another *_ref.py, no formula taken
from vk_trace.h or oracle.cpp.  From vecchio_amd only the ffi constants that name the records of a scene description.  The one exception
is the RNG stream (oracle_ffi.draws, passed in by the caller), which is not under test here.

closest_hit() walks a scene DESCRIPTION: every sphere, moving sphere, rect, list, Boxy face and FlipFace bit under any chain of
Translate / Rotate records, in the order BVHNode::hit and Vec::hit visit them (that order decides ties), with no box test anywhere: a
box can only cull what would not have been hit.  Beside the hit it returns a stability record per ray; stable() turns the record into
the rays on which an f32 evaluation has to agree with the f64 one in every discrete field.

Stability thresholds (properties of the f64 record alone, stated once, here):"""
import math

import numpy as np

from vecchio_amd import ffi

f64 = np.float64
TMIN = 0.001                       # main.rs:130
GRAZE_MIN = 1e-3                   # sqrt(disc) / (|d| r) of any sphere; |d . axis| / |d| of a rect that is met
EDGE_MIN = 1e-3                    # distance to the nearest rect edge, in units of the rect's size along that axis
GAP_MIN = 1e-4                     # (t_runner_up - t_winner) / t_winner
POLE_MAX = 0.999                   # |n . y| of the winner's object-space normal: above it v (asin) and u (atan2) are ill-conditioned
# the two below are not set by the issue; the reasoning: an f32 root t carries an error of a few ulp of (|o| + |c| + r) / |d| (the
# positions it is a difference of, over the speed), 6e-8 each: 1e-4 of that scale is three orders above it
BOUND_MIN = 1e-4                   # distance of any root from tmin or tmax, in units of (|o| + |c| + r) / |d|
FACING_MIN = 1e-3                  # |d' . n| / |d| where a Translate / Rotate re-derives `front` (hittable.rs:519, 618, 707, 796)
# the grazing margin alone does not bound the f32 discriminant's error: half_b^2 - a c is a difference of terms of size a |oc|^2, each
# carrying a few ulp (6e-8), so its SIGN is open while |disc| / (a (|oc|^2 + r^2)) = (margin r)^2 / (|oc|^2 + r^2) is a few ulp: a sphere
# of radius 0.3 seen from 13.5 away at margin 4.4e-3 has 1e-8 there, and the oracle misses it (found by this module's first run)
CANCEL_MIN = 1e-6                  # |disc| / (a (|oc|^2 + r^2)) of any sphere: 16 ulp
SEAM_MIN = 1e-3                    # distance of u from 0 / 1 (u is compared modulo 1; a texel lookup is not)
TEXEL_MIN = 1e-4                   # distance of u * width, (1 - v) * height from the next integer
CHECKER_MIN = 1e-4                 # |sin(10 x)| of each factor (f32 argument rounding at |10 x| <= 100: 4e-6)

# Float bounds: 4 x the oracle's worst deviation from the f64 value, measured on the CPU over every stable ray of every scene and ray set
# of tests/test_geometry.py (pytest -s prints each figure; DESIGN.md "Closed-form geometry" holds the table).  Never from the emulator
# or the device.
#   t          relative to t                         4.10e-5   (wild 1; the nine random graphs: 1.2e-5 .. 4.1e-5)
#   p          relative to max(|o|, t |d|)           2.34e-5   (gen 1018)
#   normal     absolute                              6.29e-4   (wild 1: a sphere met at a grazing margin just above 1e-3)
#   uv         absolute, u modulo 1                  8.02e-4   (wild 1)
#   albedo     absolute, Checker / Image at given (u, v, p)          7.43e-8
#   noise      absolute, NoiseTexture at a given p, |p| <= 9         1.31e-6
#   aov_albedo absolute, the texture at the first hit's own (u, v, p)  1.09e-4   (the noise textures follow the hit point's error)
#   camera     relative to the focus distance: vkh_camera_new's vectors and origin + direction of a camera ray     6.15e-7
MEASURED = dict(t=4.10e-5, p=2.34e-5, normal=6.29e-4, uv=8.02e-4, albedo=7.43e-8, noise=1.31e-6, aov_albedo=1.09e-4, camera=6.15e-7)
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
MAX_EXCLUDED = 0.01                # share of a scene's rays that may be unstable

KIND_SHIFT, INDEX_MASK, FLIP = 28, ffi.VK_REF_INDEX_MASK, ffi.VK_REF_FLIP


# ================================================================ a description as plain numbers
def _v(f3):
    return np.array([float(x) for x in f3], f64)


class Scene:
    """the records of a vk_scene_desc as f64 (every f32 of the description is exact in f64)"""

    def __init__(self, desc):
        d = desc.contents if hasattr(desc, "contents") else desc
        self.world = int(d.world)
        self.bvh = [(int(b.left), int(b.right)) for b in d.bvh[:d.n_bvh]]
        self.spheres = [(_v(s.center), float(s.radius), int(s.material)) for s in d.spheres[:d.n_spheres]]
        self.moving = [(_v(s.center0), _v(s.center1), float(s.time0), float(s.time1), float(s.radius), int(s.material))
                       for s in d.moving_spheres[:d.n_moving_spheres]]
        self.rects = [(float(r.c0), float(r.c1), float(r.d0), float(r.d1), float(r.k), int(r.axis0), int(r.axis1), int(r.axis2),
                       int(r.material)) for r in d.rects[:d.n_rects]]
        items = [int(x) for x in d.list_items[:d.n_list_items]]
        self.lists = [items[l.first:l.first + l.count] for l in d.lists[:d.n_lists]]
        self.media = [(int(m.boundary), float(m.neg_inv_density), int(m.material)) for m in d.media[:d.n_media]]
        self.translates = [(int(t.child), _v(t.offset)) for t in d.translates[:d.n_translates]]
        self.rotates = [(int(r.child), int(r.axis), float(r.sin_theta), float(r.cos_theta)) for r in d.rotates[:d.n_rotates]]
        self.materials = [(int(m.kind), int(m.texture), float(m.param)) for m in d.materials[:d.n_materials]]
        self.textures = [(int(t.kind), _v(t.color), int(t.a), int(t.b), float(t.scale)) for t in d.textures[:d.n_textures]]
        self.images = [np.ctypeslib.as_array(im.rgb, (int(im.height), int(im.width), 3)).copy() for im in d.images[:d.n_images]]
        self.perlins = [(np.array([[float(c) for c in row] for row in p.ranvec], f64), np.array(list(p.perm_x), np.int64),
                         np.array(list(p.perm_y), np.int64), np.array(list(p.perm_z), np.int64)) for p in d.perlins[:d.n_perlins]]


# ================================================================ hit records, n rays at a time
class Rec:
    FIELDS = ("hit", "t", "p", "normal", "front", "u", "v", "object", "material", "pole")

    def __init__(self, n):
        self.hit, self.front = np.zeros(n, bool), np.zeros(n, bool)
        self.t, self.u, self.v, self.pole = np.full(n, np.inf), np.zeros(n), np.zeros(n), np.zeros(n)
        self.p, self.normal = np.zeros((n, 3)), np.zeros((n, 3))
        self.object, self.material = np.zeros(n, np.uint32), np.zeros(n, np.uint32)

    def take(self, other, mask):
        """self where not mask, other where mask"""
        for f in Rec.FIELDS:
            a, b = getattr(self, f), getattr(other, f)
            setattr(self, f, np.where(mask[:, None] if a.ndim == 2 else mask, b, a))
        return self


class Stability:
    """what closest_hit() records about each ray beside its hit (module docstring); every entry is a minimum over the primitives"""

    def __init__(self, n, tmax):
        inf = np.full(n, np.inf)
        self.graze, self.edge, self.bound, self.facing, self.cancel = inf.copy(), inf.copy(), inf.copy(), inf.copy(), inf.copy()
        self.tmax = tmax
        self.candidates = {}           # (wrapper chain, primitive) -> t of that primitive alone within [tmin, the ray's tmax]


def _dot(a, b):
    return (a * b).sum(-1)


def _orient(d, outward):
    """HitRec::set_face_normal, hittable.rs:23-30"""
    front = _dot(d, outward) < 0.0
    return front, np.where(front[:, None], outward, -outward)


def spherical(p):
    """Sphere::spherical, hittable.rs:54-61"""
    phi = np.arctan2(p[:, 2], p[:, 0])
    theta = np.arcsin(np.clip(p[:, 1], -1.0, 1.0))
    return 1.0 - (phi + math.pi) / (2.0 * math.pi), (theta + math.pi / 2.0) / math.pi


def _sphere(center, radius, material, ref, o, d, tmin, tmax, st, key):
    """Sphere::hit, hittable.rs:65-95 (MovingSphere::hit, :154-184, with center(time)): the first root in tmin < t < tmax"""
    n = len(o)
    oc = o - center
    a, half_b, c = _dot(d, d), _dot(oc, d), _dot(oc, oc) - radius * radius
    disc = half_b * half_b - a * c
    root = np.sqrt(np.maximum(disc, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (-half_b - root) / a, (-half_b + root) / a
        length = np.sqrt(a)
        scale = (np.abs(o).max(1) + np.abs(center).max(-1) + abs(radius)) / length

        def first(hi):
            ok1 = (disc > 0.0) & (tmin < t1) & (t1 < hi)
            ok2 = (disc > 0.0) & ~ok1 & (tmin < t2) & (t2 < hi)
            return ok1 | ok2, np.where(ok1, t1, t2)

        hit, t = first(tmax)
        full_hit, full_t = first(st.tmax)
        st.candidates[key] = np.where(full_hit, full_t, np.inf)
        st.graze = np.minimum(st.graze, np.sqrt(np.abs(disc)) / (length * abs(radius)))
        st.cancel = np.minimum(st.cancel, np.abs(disc) / (a * (_dot(oc, oc) + radius * radius)))
        for r in (t1, t2):
            for b in (tmin, st.tmax):
                gap = np.where((disc > 0.0) & np.isfinite(b), np.abs(r - b) / scale, np.inf)
                st.bound = np.minimum(st.bound, gap)
    rec = Rec(n)
    t = np.where(hit, t, 0.0)
    p = o + d * t[:, None]
    outward = (p - center) / radius
    front, normal = _orient(d, outward)
    u, v = spherical(outward)
    rec.hit, rec.t, rec.p, rec.normal, rec.front, rec.u, rec.v = hit, np.where(hit, t, np.inf), p, normal, front, u, v
    rec.pole = np.abs(outward[:, 1])
    rec.object[:], rec.material[:] = ref & ~FLIP, material
    return rec


def _rect(r, ref, o, d, tmin, tmax, st, key):
    """Rect::hit, hittable.rs:230-256: tmin <= t <= tmax, the extents inclusive, the outward normal +axis2"""
    c0, c1, d0, d1, k, a0, a1, a2, material = r
    n = len(o)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (k - o[:, a2]) / d[:, a2]
        a, b = o[:, a0] + t * d[:, a0], o[:, a1] + t * d[:, a1]
        inside = ~((a < c0) | (a > c1) | (b < d0) | (b > d1))
        hit = ~((t < tmin) | (t > tmax)) & inside
        full = ~((t < tmin) | (t > st.tmax)) & inside
        st.candidates[key] = np.where(full, t, np.inf)
        # near an edge: inside the rect grown by EDGE_MIN of its size and outside the rect shrunk by as much
        ea, eb = np.minimum(np.abs(a - c0), np.abs(a - c1)) / (c1 - c0), np.minimum(np.abs(b - d0), np.abs(b - d1)) / (d1 - d0)
        fa, fb = (a - c0) / (c1 - c0), (b - d0) / (d1 - d0)
        near = (fa > -EDGE_MIN) & (fa < 1 + EDGE_MIN) & (fb > -EDGE_MIN) & (fb < 1 + EDGE_MIN) & ~((t < tmin) | (t > st.tmax))
        st.edge = np.minimum(st.edge, np.where(near, np.minimum(ea, eb), np.inf))
        length = np.sqrt(_dot(d, d))
        st.graze = np.minimum(st.graze, np.where(near, np.abs(d[:, a2]) / length, np.inf))
        scale = (np.abs(o).max(1) + abs(k)) / np.abs(d[:, a2])
        for bnd in (tmin, st.tmax):
            st.bound = np.minimum(st.bound, np.where(near & np.isfinite(bnd), np.abs(t - bnd) / scale, np.inf))
    rec = Rec(n)
    outward = np.zeros((n, 3))
    outward[:, a2] = 1.0
    t = np.where(hit, t, 0.0)
    rec.front, rec.normal = _orient(d, outward)
    rec.hit, rec.t, rec.p = hit, np.where(hit, t, np.inf), o + d * t[:, None]
    rec.u, rec.v = (a - c0) / (c1 - c0), (b - d0) / (d1 - d0)
    rec.object[:], rec.material[:] = ref & ~FLIP, material
    return rec


def _rotate(axis, s, c, x, inverse):
    """Rotate*::hit's two maps.  Forward (world to object, hittable.rs:591-595 Y, :680-684 X, :769-773 Z) and back (:603-607, :692-696,
    :781-785).  Y mixes (x, z) with the sine's sign the other way round from X's (y, z) and Z's (x, y), as the reference has it."""
    i, j = ((1, 2), (0, 2), (0, 1))[axis]
    sign = -1.0 if axis == 1 else 1.0            # forward: X  y' =  c y + s z, z' = -s y + c z;  Y  x' = c x - s z, z' = s x + c z
    if inverse:
        sign = -sign
    out = x.copy()
    out[:, i] = c * x[:, i] + sign * s * x[:, j]
    out[:, j] = -sign * s * x[:, i] + c * x[:, j]
    return out


def _hit(sc, ref, o, d, time, tmin, tmax, st, chain=()):
    kind, index = ref >> KIND_SHIFT, ref & INDEX_MASK
    n = len(o)
    if kind == ffi.VK_KIND_SPHERE:
        center, radius, material = sc.spheres[index]
        rec = _sphere(center, radius, material, ref, o, d, tmin, tmax, st, (chain, ref & ~FLIP))
    elif kind == ffi.VK_KIND_MOVING_SPHERE:
        c0, c1, t0, t1, radius, material = sc.moving[index]
        center = c0 + (c1 - c0) * ((time - t0) / (t1 - t0))[:, None]           # MovingSphere::center, hittable.rs:147-150: no clamp
        rec = _sphere(center, radius, material, ref, o, d, tmin, tmax, st, (chain, ref & ~FLIP))
    elif kind == ffi.VK_KIND_RECT:
        rec = _rect(sc.rects[index], ref, o, d, tmin, tmax, st, (chain, ref & ~FLIP))
    elif kind == ffi.VK_KIND_LIST:
        # Vec::hit, hittable.rs:381-394: every item against the closest so far, replaced only by a strictly smaller t
        rec, closest = Rec(n), tmax.copy()
        for item in sc.lists[index]:
            r = _hit(sc, item, o, d, time, tmin, closest, st, chain)
            better = r.hit & (r.t < closest)
            closest = np.where(better, r.t, closest)
            rec.take(r, better)
    elif kind == ffi.VK_KIND_BVH:
        # BVHNode::hit, accel.rs:64-82, without the box test: the right child against the left one's t; of two hits the left one only
        # where its t is strictly smaller
        left, right = sc.bvh[index]
        rec = _hit(sc, left, o, d, time, tmin, tmax, st, chain)
        r = _hit(sc, right, o, d, time, tmin, np.where(rec.hit, rec.t, tmax), st, chain)
        rec.take(r, r.hit & ~(rec.hit & (rec.t < r.t)))
    elif kind == ffi.VK_KIND_TRANSLATE:
        # Translate::hit, hittable.rs:507-523: set_face_normal on the child's ALREADY ORIENTED normal
        child, off = sc.translates[index]
        rec = _hit(sc, child, o - off, d, time, tmin, tmax, st, chain + (ref & ~FLIP,))
        rec.p = rec.p + off
        _reface(rec, d, d, st)
    elif kind == ffi.VK_KIND_ROTATE:
        # Rotate*::hit: the WORLD-space normal oriented against the OBJECT-space ray, hittable.rs:618, 707, 796
        child, axis, s, c = sc.rotates[index]
        d_obj = _rotate(axis, s, c, d, False)
        rec = _hit(sc, child, _rotate(axis, s, c, o, False), d_obj, time, tmin, tmax, st, chain + (ref & ~FLIP,))
        rec.p, rec.normal = _rotate(axis, s, c, rec.p, True), _rotate(axis, s, c, rec.normal, True)
        _reface(rec, d_obj, d, st)
    else:
        raise ValueError(f"closest_hit: no closed form for a record of kind {kind} here (media: medium_segment())")
    if ref & FLIP:
        rec.front = ~rec.front                                                    # FlipFace::hit, hittable.rs:299-308
    return rec


def _reface(rec, d_used, d, st):
    facing = _dot(d_used, rec.normal)
    st.facing = np.minimum(st.facing, np.where(rec.hit, np.abs(facing) / np.sqrt(_dot(d, d)), np.inf))
    rec.front, rec.normal = _orient(d_used, rec.normal)


HIT_FIELDS = ("hit", "t", "p", "normal", "front", "u", "v", "object", "material")


def closest_hit(sc, origin, direction, time=0.0, tmax=np.inf, world=None):
    """world.hit(r, 0.001, tmax) (main.rs:130) for n rays: (hit dict, stability dict).  A miss is hit = 0, t = +inf, everything else 0;
    a ray whose tmax is a NaN or <= 0.001 misses (the interface's own rule, include/vecchio_amd.h)."""
    o, d = np.asarray(origin, f64).reshape(-1, 3), np.asarray(direction, f64).reshape(-1, 3)
    n = len(o)
    time = np.broadcast_to(np.asarray(time, f64), (n,)).astype(f64)
    tmax = np.broadcast_to(np.asarray(tmax, f64), (n,)).astype(f64)
    live = tmax > TMIN
    tm = np.where(live, tmax, TMIN)
    st = Stability(n, tm)
    rec = _hit(sc, sc.world if world is None else world, o, d, time, np.full(n, TMIN), tm, st)
    hit = rec.hit & live
    out = {}
    for f in HIT_FIELDS:
        a = getattr(rec, f)
        out[f] = np.where(hit[:, None] if a.ndim == 2 else hit, a, np.inf if f == "t" else 0).astype(a.dtype)
    ts = np.sort(np.stack(list(st.candidates.values())), axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (ts[1] - ts[0]) / np.abs(ts[0]) if len(ts) > 1 else np.full(n, np.inf)
    gap = np.where(np.isfinite(ts[0]), np.where(np.isnan(gap), np.inf, gap), np.inf)
    seam = np.where(hit, np.minimum(rec.u % 1.0, 1.0 - rec.u % 1.0), np.inf)
    degenerate = ~(np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0.0).all(1)) | ~live
    record = dict(graze=st.graze, cancel=st.cancel, edge=st.edge, gap=gap, bound=st.bound, facing=st.facing, pole=np.where(hit, rec.pole, 0.0), seam=seam,
                  degenerate=degenerate)
    return out, record


def stable(record):
    """the rays on which every discrete field of an f32 evaluation has to equal the f64 one"""
    return ((record["graze"] >= GRAZE_MIN) & (record["cancel"] >= CANCEL_MIN) & (record["edge"] >= EDGE_MIN) & (record["gap"] >= GAP_MIN) & (record["bound"] >= BOUND_MIN) &
            (record["facing"] >= FACING_MIN) & ~record["degenerate"])


def uv_stable(record):
    """of the stable rays, those whose u and v are well-conditioned too (away from the poles)"""
    return stable(record) & (record["pole"] <= POLE_MAX)


# ================================================================ ConstantMedium
def medium_segment(sc, medium, origin, direction, time=0.0, tmin=TMIN, tmax=np.inf):
    """ConstantMedium::hit, hittable.rs:457-472, up to the draw: (valid, t_in, t_out, length) — the boundary met from -inf, met again
    from t + 0.0001, the pair clipped to [tmin, tmax] and to t >= 0, and the length in units of distance, (t_out - t_in) |d|"""
    o, d = np.asarray(origin, f64).reshape(-1, 3), np.asarray(direction, f64).reshape(-1, 3)
    n = len(o)
    time = np.broadcast_to(np.asarray(time, f64), (n,)).astype(f64)
    boundary = sc.media[medium][0]
    inf = np.full(n, np.inf)
    rec1 = _hit(sc, boundary, o, d, time, -inf, inf, Stability(n, inf))
    rec2 = _hit(sc, boundary, o, d, time, np.where(rec1.hit, rec1.t, 0.0) + 0.0001, inf, Stability(n, inf))
    t1, t2 = np.maximum(rec1.t, tmin), np.minimum(rec2.t, tmax)
    valid = rec1.hit & rec2.hit & (t1 < t2)
    t1 = np.maximum(t1, 0.0)
    return valid, t1, t2, (t2 - t1) * np.sqrt(_dot(d, d))


def medium_density(sc, medium):
    return -1.0 / sc.media[medium][1]                  # ConstantMedium::new, hittable.rs:447


def scatter_probability(density, length):
    """hit_distance = -ln(xi) / density <= length (hittable.rs:473-476), xi uniform: 1 - exp(-density length)"""
    return -np.expm1(-density * length)


def scatter_moments(density, length):
    """(E s, E s^2) of the scatter distance s = (t - t_in) |d| (hittable.rs:479) given that the ray scatters: the exponential law of
    rate `density` truncated to [0, length]"""
    r, L = density, length
    P, e = -np.expm1(-r * L), np.exp(-r * L)
    return (1.0 / r - e * (L + 1.0 / r)) / P, (2.0 / r ** 2 - e * (L * L + 2.0 * L / r + 2.0 / r ** 2)) / P


# ================================================================ textures
def _usize(x):
    """`f32 as usize` (material.rs:399-401): saturating — a negative value and a NaN give 0"""
    x = np.where(np.isnan(x), 0.0, x)
    return np.clip(x, 0.0, 2.0 ** 62).astype(np.int64)


def perlin_noise(perlin, p):
    """Perlin::noise, material.rs:392-413, and perlin_interp, :331-352"""
    ranvec, px, py, pz = perlin
    fl = np.floor(p)
    uvw = p - fl
    ijk = _usize(fl)
    hh = uvw * uvw * (3.0 - 2.0 * uvw)
    accum = np.zeros(len(p))
    for di in range(2):
        for dj in range(2):
            for dk in range(2):
                c = ranvec[px[(ijk[:, 0] + di) & 255] ^ py[(ijk[:, 1] + dj) & 255] ^ pz[(ijk[:, 2] + dk) & 255]]
                w = uvw - np.array([di, dj, dk], f64)
                accum += ((di * hh[:, 0] + (1 - di) * (1 - hh[:, 0])) * (dj * hh[:, 1] + (1 - dj) * (1 - hh[:, 1])) *
                          (dk * hh[:, 2] + (1 - dk) * (1 - hh[:, 2])) * _dot(c, w))
    return accum


def turb(perlin, p, depth=7):
    """Perlin::turb, material.rs:379-390"""
    accum, weight, q = np.zeros(len(p)), 1.0, np.array(p, f64)
    for _ in range(depth):
        accum += weight * perlin_noise(perlin, q)
        weight *= 0.5
        q = q * 2.0
    return np.abs(accum)


def texture_value(sc, texture, u, v, p):
    """Texture::value, material.rs:228-434: (rgb (n, 3), margin (n,)) — margin: how far each point is from a discrete decision of the
    texture (a checker's sign, a texel's border), in the units of CHECKER_MIN / TEXEL_MIN scaled to 1: >= 1 is stable"""
    u, v, p = np.asarray(u, f64).reshape(-1), np.asarray(v, f64).reshape(-1), np.asarray(p, f64).reshape(-1, 3)
    n = len(u)
    kind, color, a, b, scale = sc.textures[texture]
    if kind == ffi.VK_TEX_SOLID:                                                   # :238-242
        return np.tile(color, (n, 1)), np.full(n, np.inf)
    if kind == ffi.VK_TEX_CHECKER:                                                 # :250-258: odd where the product of sines < 0
        sines = np.sin(10.0 * p)
        odd, m_odd = texture_value(sc, a, u, v, p)
        even, m_even = texture_value(sc, b, u, v, p)
        neg = sines.prod(1) < 0.0
        margin = np.minimum(np.abs(sines).min(1) / CHECKER_MIN, np.where(neg, m_odd, m_even))
        return np.where(neg[:, None], odd, even), margin
    if kind == ffi.VK_TEX_IMAGE:                                                   # :283-303: clamp, v flipped, truncation, clamp
        img = sc.images[a]
        h, w = img.shape[:2]
        x, y = np.clip(u, 0.0, 1.0) * w, (1.0 - np.clip(v, 0.0, 1.0)) * h
        i, j = np.minimum(_usize(x), w - 1), np.minimum(_usize(y), h - 1)
        frac = lambda q, size: np.where((q <= 0.0) | (q >= size), np.inf, np.minimum(q - np.floor(q), np.ceil(q) - q))
        margin = np.minimum(frac(x, w), frac(y, h)) / TEXEL_MIN
        return img[j, i].astype(f64) * (1.0 / 255.0), margin
    if kind == ffi.VK_TEX_NOISE:                                                   # :430-433
        val = 0.5 * (1.0 + np.sin(scale * p[:, 2] + 10.0 * turb(sc.perlins[a], p, 7)))
        return np.repeat(val[:, None], 3, 1), np.full(n, np.inf)
    raise ValueError(f"texture kind {kind}")


def albedo_of(sc, hit):
    """the first-hit albedo of a Lambertian carrier: its texture at (u, v, p) of the hit (material.rs:85-108); 0 where nothing is hit"""
    n = len(hit["t"])
    rgb, margin = np.zeros((n, 3)), np.full(n, np.inf)
    for m in np.unique(hit["material"][hit["hit"]]):
        sel = hit["hit"] & (hit["material"] == m)
        rgb[sel], margin[sel] = texture_value(sc, sc.materials[m][1], hit["u"][sel], hit["v"][sel], hit["p"][sel])
    return rgb, margin


# ================================================================ camera
def camera_new(lookfrom, lookat, vup, vfov, aspect, aperture, focus, time0=0.0, time1=1.0):
    """Camera::new, main.rs:71-109"""
    lookfrom, lookat, vup = (np.asarray(x, f64) for x in (lookfrom, lookat, vup))
    h = math.tan(math.radians(vfov) / 2.0)
    vh = 2.0 * h
    vw = aspect * vh
    w = (lookfrom - lookat) / np.linalg.norm(lookfrom - lookat)
    u = np.cross(vup, w)
    u = u / np.linalg.norm(u)
    v = np.cross(w, u)
    hor, ver = u * vw * focus, v * vh * focus
    return dict(origin=lookfrom, horizontal=hor, vertical=ver, lower_left_corner=lookfrom - hor / 2.0 - ver / 2.0 - w * focus, u=u, v=v, w=w,
                lens_radius=aperture / 2.0, time0=float(time0), time1=float(time1))


def pixel_st(xi, x, y, width, height):
    """main.rs:187-188: s = (x + xi0) / (width - 1), t = (y + xi1) / (height - 1) from the stream's first two draws"""
    xi = np.asarray(xi, f64)
    return (x + xi[..., 0]) / (width - 1), (y + xi[..., 1]) / (height - 1)


def focus_point(cam, s, t):
    """origin + direction of Camera::get_ray, main.rs:115-118: lower_left + s horizontal + t vertical, whatever the lens offset"""
    s, t = np.asarray(s, f64), np.asarray(t, f64)
    return cam["lower_left_corner"] + s[..., None] * cam["horizontal"] + t[..., None] * cam["vertical"]


def lens_coordinates(cam, origin):
    """(a, b, c) of a ray origin: origin - lookfrom = a u + b v + c w.  get_ray (main.rs:113-116) needs a^2 + b^2 < lens_radius^2
    (random_in_unit_disk is strictly inside) and c = 0."""
    off = np.asarray(origin, f64) - cam["origin"]
    return off @ cam["u"], off @ cam["v"], off @ cam["w"]


def stream_draws(draws, seed, width, height, spp, first_sample=0):
    """(height, width, spp, 2): the first two draws of every sample's stream, stream (seed, pixel = y width + x, sample) (main.rs:182-188);
    draws: oracle_ffi.draws"""
    out = np.zeros((height, width, spp, 2))
    for y in range(height):
        for x in range(width):
            for k in range(spp):
                out[y, x, k] = draws(seed, y * width + x, first_sample + k, 0, 2)
    return out


# ================================================================ holding an f32 evaluation to the closed forms
def rays_f64(rays):
    """(origin, direction, time, tmax) in f64 of vk_ray records"""
    return rays["origin"].astype(f64), rays["direction"].astype(f64), rays["time"].astype(f64), rays["tmax"].astype(f64)


def reference(sc, rays):
    """(hit, record) of closest_hit() for vk_ray records"""
    return closest_hit(sc, *rays_f64(rays))


def compare_hits(got, want, record, rays, what):
    """got: vk_hit records of an f32 evaluation; want, record: closest_hit()'s.  hit, front, material, object and medium exact on every
    stable ray, at most MAX_EXCLUDED of the rays unstable; returns the worst float deviations over the stable hits (t relative, p relative
    to max(|o|, t |d|), normal, v and u modulo 1 absolute; u and v on the rays away from the poles) and the excluded share."""
    ok, uv_ok = stable(record), uv_stable(record)
    excluded = 1.0 - ok.mean()
    assert excluded <= MAX_EXCLUDED, f"{what}: {excluded:.4f} of the rays are unstable (cap {MAX_EXCLUDED})"
    for f in ("hit", "front", "material", "object"):
        bad = np.flatnonzero(ok & (got[f].astype(np.int64) != want[f].astype(np.int64)))
        assert len(bad) == 0, (f"{what}: {f} differs on {len(bad)} stable rays; first {bad[0]}: got {got[bad[0]]}, want "
                               + str({k: want[k][bad[0]] for k in HIT_FIELDS}) + " record " + str({k: record[k][bad[0]] for k in record}))
    assert not got["medium"][ok].any(), f"{what}: a medium hit in a scene without media"
    h = ok & want["hit"]
    o, d, _, _ = rays_f64(rays)
    worst = dict(t=0.0, p=0.0, normal=0.0, uv=0.0, excluded=excluded, hits=int(h.sum()))
    if h.any():
        t = want["t"][h]
        worst["t"] = float(np.abs(got["t"][h].astype(f64) / t - 1.0).max())
        scale = np.maximum(np.linalg.norm(o[h], axis=1), t * np.linalg.norm(d[h], axis=1))
        worst["p"] = float((np.abs(got["p"][h].astype(f64) - want["p"][h]).max(1) / scale).max())
        worst["normal"] = float(np.abs(got["normal"][h].astype(f64) - want["normal"][h]).max())
    # u and v are compared away from the poles only: that further exclusion has the same cap
    worst["uv_excluded"] = float((ok & want["hit"] & ~uv_ok).mean())
    assert worst["uv_excluded"] <= MAX_EXCLUDED, f"{what}: {worst['uv_excluded']:.4f} of the rays hit within |n . y| > {POLE_MAX} of a pole"
    h = uv_ok & want["hit"]
    if h.any():
        du = np.abs(got["u"][h].astype(f64) - want["u"][h]) % 1.0
        worst["uv"] = float(max(np.minimum(du, 1.0 - du).max(), np.abs(got["v"][h].astype(f64) - want["v"][h]).max()))
    return worst


def assert_within(worst, what, bound=None):
    bound = bound or BOUND
    for k in ("t", "p", "normal", "uv"):
        assert worst[k] <= bound[k], f"{what}: {k} deviates by {worst[k]:.3g} from the f64 value, bound {bound[k]:.3g}"
