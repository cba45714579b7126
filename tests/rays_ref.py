"""Reference for ray queries (vk_trace_rays): one oracle_hit per ray, and the ray sets the emulator and the device tests share.  TESTS ONLY.

oracle_hit names neither the primitive it hit nor whether a ConstantMedium filled the record.  So the reference runs on a COPY of the
description in which every sphere, moving sphere, rect and medium record has a duplicate of its material all to itself (tagged()): the
geometry, the tree and every result are unchanged — nothing in a hit depends on a material's index — and the material index the oracle
reports then names the record whose own hit() produced the winner, for every hit of every scene.  The original index, `object` and `medium`
are read from the duplicate's entry in the table.

The two rules that are the interface's own (include/vecchio_amd.h), not the oracle's: a ray whose tmax is a NaN or <= 0.001 misses, and a
miss is hit = 0, t = +inf, everything else 0."""
import ctypes as C

import numpy as np

from vecchio_amd import ffi
from vecchio_amd.scene import HIT_DTYPE, make_rays

f32 = np.float32
GOLDEN = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def ray_seed(seed, index):
    """the stream of ray `index` of a batch: seed + GOLDEN * index in wrapping u64"""
    return (seed + GOLDEN * index) & MASK


def tagged(desc):
    """(description pointer, owner): the copy with one material per primitive record.  owner[i - n_materials] = (vk_ref without flip,
    original material, is_medium) for duplicate i.  The returned pointer keeps its arrays alive through attributes of the struct."""
    src = desc.contents
    d = ffi.SceneDesc.from_buffer_copy(src)
    mats = [ffi.Material.from_buffer_copy(src.materials[i]) for i in range(src.n_materials)]
    owner = []

    def retag(T, n, ptr, kind):
        recs = [T.from_buffer_copy(ptr[i]) for i in range(n)]
        for i, r in enumerate(recs):
            owner.append((ffi.make_ref(kind, i), r.material, kind == ffi.VK_KIND_MEDIUM))
            mats.append(ffi.Material.from_buffer_copy(src.materials[r.material]))
            r.material = len(mats) - 1
        return (T * max(1, n))(*recs)

    spheres = retag(ffi.Sphere, src.n_spheres, src.spheres, ffi.VK_KIND_SPHERE)
    moving = retag(ffi.MovingSphere, src.n_moving_spheres, src.moving_spheres, ffi.VK_KIND_MOVING_SPHERE)
    rects = retag(ffi.Rect, src.n_rects, src.rects, ffi.VK_KIND_RECT)
    media = retag(ffi.Medium, src.n_media, src.media, ffi.VK_KIND_MEDIUM)
    marr = (ffi.Material * len(mats))(*mats)
    d.spheres, d.moving_spheres, d.rects, d.media = spheres, moving, rects, media
    d.materials, d.n_materials = marr, len(mats)
    d._keep = (spheres, moving, rects, media, marr, desc)
    assert len(mats) < (1 << 24), "oracle_hit reports the material index as a float"
    return C.pointer(d), owner


def ref_hits(oracle, desc, rays, seed=0, first_index=0, _tagged=None):
    """the HIT_DTYPE array vk_trace_rays must return for `rays` (RAY_DTYPE)"""
    tdesc, owner = _tagged or tagged(desc)
    n_mat = desc.contents.n_materials
    out = np.zeros(len(rays), HIT_DTYPE)
    out["t"] = np.inf
    for i, r in enumerate(rays):
        tmax = float(r["tmax"])
        if not tmax > 0.001:                   # (a NaN too)
            continue
        h = oracle.hit(tdesc, [float(x) for x in r["origin"]], [float(x) for x in r["direction"]], float(r["time"]), 0.001, tmax,
                       ray_seed(seed, first_index + i))
        if h is None:
            continue
        assert h["material"] >= n_mat, "a hit on a record that has no duplicate material"
        ref, mat, is_medium = owner[h["material"] - n_mat]
        o = out[i]
        o["p"], o["normal"], o["t"], o["u"], o["v"] = h["p"], h["normal"], h["t"], h["u"], h["v"]
        o["hit"], o["front"], o["material"], o["object"], o["medium"] = 1, int(h["front"]), mat, ref, int(is_medium)
    return out


# ---------------------------------------------------------------- ray sets
def _interesting_points(desc):
    """centres of glass spheres and of media (sphere or Boxy boundaries), in the coordinates the records are written in"""
    d = desc.contents
    pts = []
    for i in range(d.n_spheres):
        s = d.spheres[i]
        if d.materials[s.material].kind == ffi.VK_MAT_DIELECTRIC:
            pts.append((list(s.center), abs(s.radius)))
    for i in range(d.n_media):
        b = d.media[i].boundary
        k, j = b >> 28, b & 0x07FFFFFF
        if k == ffi.VK_KIND_SPHERE:
            pts.append((list(d.spheres[j].center), abs(d.spheres[j].radius)))
        elif k == ffi.VK_KIND_LIST and d.lists[j].count == 6:
            q = [d.rects[d.list_items[d.lists[j].first + f] & 0x07FFFFFF] for f in range(2)]
            pts.append(([(q[0].c0 + q[0].c1) / 2, (q[0].d0 + q[0].d1) / 2, (q[0].k + q[1].k) / 2], abs(q[0].k - q[1].k) / 2))
    return pts[:6]


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def ray_sets(oracle, desc, cam, p, rng_seed=1):
    """name -> RAY_DTYPE array: the sets of the issue, from a seeded generator"""
    rng = np.random.default_rng(rng_seed)
    fh = oracle.first_hits(desc, cam, p, 0, 1).reshape(-1)
    sets = {}
    sets["primary"] = make_rays(fh["origin"], fh["direction"], fh["time"])
    hit = fh[fh["hit"] == 1]
    pts = hit["p"][np.isfinite(hit["p"]).all(1)]
    lo = np.clip(pts.min(0), -2000, 2000) if len(pts) else f32([-5, -5, -5])
    hi = np.clip(pts.max(0), -2000, 2000) if len(pts) else f32([5, 5, 5])
    ctr, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 0.5)
    t0, t1 = float(cam.time0), float(cam.time1)
    n = 96
    # through the world box from outside ...
    target = (ctr + half * rng.uniform(-1, 1, (n, 3))).astype(f32)
    origin = (ctr + 3.0 * np.linalg.norm(half) * _unit(rng, n)).astype(f32)
    sets["outside"] = make_rays(origin, target - origin, rng.uniform(t0, t1, n))
    # ... and from inside, in any direction and of any length
    origin = (ctr + half * rng.uniform(-1, 1, (n, 3))).astype(f32)
    sets["inside"] = make_rays(origin, _unit(rng, n) * rng.uniform(0.01, 30, (n, 1)).astype(f32), rng.uniform(t0, t1, n))
    # from inside glass spheres and media
    special = _interesting_points(desc)
    if special:
        o, d = [], []
        for c, r in special:
            k = 16
            o.append(f32(c) + f32(0.5 * r) * _unit(rng, k) * rng.uniform(0, 1, (k, 1)).astype(f32))
            d.append(_unit(rng, k))
        sets["inside_glass_and_media"] = make_rays(np.concatenate(o), np.concatenate(d), rng.uniform(t0, t1, 16 * len(special)))
    if len(hit):
        # restarted at first-hit points: the mirror direction, and straight on (through glass, out of a medium)
        h = hit[:: max(1, len(hit) // 64)][:64]
        dd, nn = h["direction"], h["normal"]
        refl = (dd - f32(2) * (dd * nn).sum(1, keepdims=True).astype(f32) * nn).astype(f32)
        sets["restarts"] = np.concatenate([make_rays(h["p"], refl, h["time"]), make_rays(h["p"], dd, h["time"])])
        # tmax just before, exactly at and just after a known hit
        h = hit[:: max(1, len(hit) // 48)][:48]
        cuts = []
        for t in (np.nextafter(h["t"], f32(-np.inf)), h["t"], np.nextafter(h["t"], f32(np.inf))):
            cuts.append(make_rays(h["origin"], h["direction"], h["time"], t))
        sets["tmax_cuts"] = np.concatenate(cuts)
    # axis-parallel, zero-direction, NaN and infinite rays; tmax that is a NaN, tmin itself, negative
    eye = f32(list(cam.origin))
    o, d, tm = [], [], []
    for org in (eye, ctr.astype(f32)):
        for axis in range(3):
            for sgn in (1.0, -1.0):
                v = np.zeros(3, f32)
                v[axis] = sgn
                o.append(org); d.append(v); tm.append(np.inf)
        o.append(org); d.append(np.zeros(3, f32)); tm.append(np.inf)
    look = (ctr - eye).astype(f32)
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            v = look.copy(); v[axis] = bad
            o.append(eye); d.append(v); tm.append(np.inf)
            w = eye.copy(); w[axis] = bad
            o.append(w); d.append(look); tm.append(np.inf)
    for t in (np.nan, 0.001, 0.0, -1.0, -np.inf, 1e-3 * 1.0001):
        o.append(eye); d.append(look); tm.append(t)
    sets["odd"] = make_rays(np.array(o, f32), np.array(d, f32), t0, np.array(tm, f32))
    return sets


def all_rays(sets):
    """the sets as one batch, and each set's slice of it"""
    at, where = 0, {}
    for k, v in sets.items():
        where[k] = slice(at, at + len(v))
        at += len(v)
    return np.concatenate(list(sets.values())), where


WORDS = [(n, HIT_DTYPE.fields[n][1] // 4, int(np.prod(HIT_DTYPE.fields[n][0].shape or (1,)))) for n in HIT_DTYPE.names]


def words(hits):
    """(n, 16) uint32 view of a HIT_DTYPE array"""
    return np.ascontiguousarray(hits).view(np.uint32).reshape(-1, 16)


def assert_bit_identical(got, want, what=""):
    """every field of every ray bit for bit; a NaN equals a NaN whatever its payload (IEEE 754 leaves the payload of an operation's
    NaN result open)"""
    g, w = words(got), words(want)
    gf, wf = g.view(f32), w.view(f32)
    both_nan = np.zeros(g.shape, bool)
    both_nan[:, :9] = np.isnan(gf[:, :9]) & np.isnan(wf[:, :9])
    bad = (g != w) & ~both_nan
    if bad.any():
        i = int(np.argwhere(bad.any(1))[0, 0])
        raise AssertionError(f"{what}: {int(bad.any(1).sum())} of {len(g)} rays differ; first ray {i}:\n  got  {got[i]}\n  want {want[i]}")
