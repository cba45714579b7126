"""Per-sample references for the first-hit buffers (vk_render_aov), built from the CPU oracle.  TESTS ONLY.

(a) rays and hits, for every scene: oracle_first_hits (oracle/oracle.h) runs the radiance sample loop up to and including its first
    world.hit — the sample's own stream, the jitter and camera draws, then the hit call whose ConstantMedium draws continue that stream —
    and returns the ray, the hit record and whether ConstantMedium::hit filled it.  From those, by the rules of include/vecchio_amd.h:
    coverage; depth f32(t) * sqrt(f32(d.d)); the normal, (0,0,0) for a medium hit; the albedo from the material and the oracle's own
    Texture::value (oracle_texture_values: solid, checker, image and noise alike), the phase function's texture for a medium hit.
    primary_ray restates the camera draws in numpy float32 from the bare draw stream (oracle_draws): tests/test_aov_emu.py pins
    oracle_first_hits' rays to it bit for bit.
(b) emitter substitution, for albedo on every scene, media included: every material becomes a DiffuseLight whose emit texture is its
    albedo texture ((1,1,1) for Dielectric, a solid mix for a SpecDiffuse of solids, the emit colour clamped to [0, 1] for a light), and
    the oracle renders it with the SCATTER integrator: per sample the radiance is then the texture value at the first hit, or the
    background.  Back faces emit 0, so a second copy with VK_REF_FLIP toggled on every primitive and medium reference (black background)
    is added sample by sample.  Translate / Rotate refs are toggled too: an instance sets the face again from its own ray
    (set_face_normal, hittable.rs:507-524), so only the outermost wrapper's flip decides the face of a hit inside it.
"""
import ctypes as C

import numpy as np

from vecchio_amd import ffi

f32 = np.float32
CHANNELS = ("albedo", "normal", "depth", "coverage")


# ---------------------------------------------------------------- (a) the primary ray of sample s
class _Draws:
    """the sample's stream, one u32 per draw: gen_f32 gives u >> 8, from which every draw kind follows"""

    def __init__(self, oracle, seed, pixel, s, n=64):
        g = oracle.draws(seed, pixel, s, 0, n)
        self.hi24 = (g.astype(np.float64) * 16777216.0).astype(np.uint32)
        self.k = 0

    def _next(self):
        v = self.hi24[self.k]
        self.k += 1
        return v

    def f32(self):
        return f32(self._next()) * f32(1.0 / 16777216.0)

    def _v01(self):
        bits = np.uint32((int(self._next()) >> 1) | 0x3F800000)
        return np.array(bits, dtype=np.uint32).view(np.float32)[()] - f32(1.0)

    def pm1(self):
        return self._v01() * f32(2.0) + f32(-1.0)

    def range(self, lo, hi):
        lo, hi = f32(lo), f32(hi)
        scale = hi - lo
        if not (scale > 0) or scale > f32(3.0e38):
            return lo
        while True:
            res = self._v01() * scale + lo
            if res < hi:
                return res


def primary_ray(oracle, cam, p, x, y, s):
    """start_sample_core (vk_trace.h) in float32: origin, direction, time"""
    dr = _Draws(oracle, p.seed, y * p.width + x, s)
    u = (f32(x) + dr.f32()) / f32(p.width - 1)
    v = (f32(y) + dr.f32()) / f32(p.height - 1)
    while True:
        px, py = dr.pm1(), dr.pm1()
        if not (px * px + py * py + f32(0.0) * f32(0.0) >= f32(1.0)):
            break
    lr = f32(cam.lens_radius)
    rdx, rdy = px * lr, py * lr
    cu, cv = np.array(list(cam.u), f32), np.array(list(cam.v), f32)
    org = np.array(list(cam.origin), f32)
    offset = cu * rdx + cv * rdy
    o = org + offset
    d = np.array(list(cam.lower_left_corner), f32) + np.array(list(cam.horizontal), f32) * u + np.array(list(cam.vertical), f32) * v
    d = d - org - offset
    t = dr.range(cam.time0, cam.time1)
    return o, d, t


def _clamp01(a):
    a = np.asarray(a, f32)
    return np.where(a < 0, f32(0), np.where(a > 1, f32(1), a)).astype(f32)


def _length(d):
    """sqrt(f32(d.d)) of direction(s) d (..., 3), the products summed in x, y, z order"""
    d = np.asarray(d, f32)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], dtype=f32)


def background(p, d):
    """the background the radiance sample sees along direction(s) d (..., 3), clamped to [0, 1]"""
    d = np.asarray(d, f32)
    if p.background == ffi.VK_BACKGROUND_SKY:
        t = f32(0.5) * (d[..., 1] / _length(d) + f32(1.0))
        return _clamp01((f32(1.0) - t)[..., None] * np.array([1, 1, 1], f32) + t[..., None] * np.array([0.5, 0.7, 1.0], f32))
    return np.broadcast_to(_clamp01(list(p.background_color)), d.shape).copy()


def _albedo_a(oracle, desc_ptr, mi, fh, level=0):
    """albedo (n, 3) of material mi at the n hit records fh (material.rs; include/vecchio_amd.h vk_render_aov)"""
    desc = desc_ptr.contents
    m = desc.materials[mi]
    n = fh.shape[0]
    if m.kind == ffi.VK_MAT_DIELECTRIC:
        return np.ones((n, 3), f32)
    if m.kind == ffi.VK_MAT_SPEC_DIFFUSE:
        if level >= 8:
            return np.zeros((n, 3), f32)
        a, b = _albedo_a(oracle, desc_ptr, m.a, fh, level + 1), _albedo_a(oracle, desc_ptr, m.b, fh, level + 1)
        pct = f32(m.param)
        return (pct * a + (f32(1.0) - pct) * b).astype(f32)
    v = oracle.texture_values(desc_ptr, m.texture, fh["u"], fh["v"], fh["p"])
    if m.kind == ffi.VK_MAT_DIFFUSE_LIGHT:           # emitted(): front faces only (material.rs:218-225), clamped
        return np.where((fh["front"] != 0)[:, None], _clamp01(v), f32(0.0)).astype(f32)
    return v


def ref_a(oracle, desc_ptr, cam, p, samples):
    """per sample of `samples` and pixel: dict of arrays — coverage (0/1), depth (inf on a miss), normal, albedo, each of shape
    (len(samples), h, w[, 3]); 'medium' (bool: the first hit is a ConstantMedium's) and 'dropped' (bool: a non-finite component, the
    sample adds to no sum); 'origin', 'direction', 'time': the primary ray"""
    n = len(samples)
    shape = (n, p.height, p.width)
    fh = np.zeros(shape, dtype=oracle.FIRST_HIT_DTYPE)
    for k, s in enumerate(samples):
        fh[k] = oracle.first_hits(desc_ptr, cam, p, s, 1)[:, :, 0]
    hit = fh["hit"] != 0
    medium = hit & (fh["medium"] != 0)
    d = fh["direction"]
    albedo = np.full(shape + (3,), np.nan, f32)
    albedo[~hit] = background(p, d[~hit])
    for mi in np.unique(fh["material"][hit]):
        sel = hit & (fh["material"] == mi)
        albedo[sel] = _albedo_a(oracle, desc_ptr, int(mi), fh[sel])
    normal = np.where((hit & ~medium)[..., None], fh["normal"], f32(0.0)).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        depth = np.where(hit, fh["t"] * _length(d), f32(np.inf)).astype(f32)
    ok = np.isfinite(albedo).all(-1) & np.isfinite(normal).all(-1) & (~hit | np.isfinite(depth))
    return dict(albedo=albedo, normal=normal, depth=depth, coverage=hit.astype(f32), medium=medium, dropped=~ok,
                origin=fh["origin"].copy(), direction=d.copy(), time=fh["time"].copy(), material=fh["material"].copy())


# ---------------------------------------------------------------- (b) emitter substitution
def _solid_mix(desc, mi, level=0):
    """the albedo of material mi as a constant colour, if it is one (solid textures, Dielectric, lights, SpecDiffuse of those)"""
    m = desc.materials[mi]
    if m.kind == ffi.VK_MAT_DIELECTRIC:
        return np.ones(3, f32)
    if m.kind == ffi.VK_MAT_SPEC_DIFFUSE:
        if level >= 8:
            return np.zeros(3, f32)
        a, b = _solid_mix(desc, m.a, level + 1), _solid_mix(desc, m.b, level + 1)
        if a is None or b is None:
            return None
        pct = f32(m.param)
        return (pct * a + (f32(1.0) - pct) * b).astype(f32)
    t = desc.textures[m.texture]
    if t.kind != ffi.VK_TEX_SOLID:
        return None
    c = np.array(list(t.color), f32)
    return _clamp01(c) if m.kind == ffi.VK_MAT_DIFFUSE_LIGHT else c


class _Sub:
    """a copy of a description with every material an emitter of its albedo (and, flipped, every primitive / medium ref toggled)"""

    PRIM_KINDS = (ffi.VK_KIND_SPHERE, ffi.VK_KIND_MOVING_SPHERE, ffi.VK_KIND_RECT, ffi.VK_KIND_MEDIUM, ffi.VK_KIND_TRANSLATE,
                  ffi.VK_KIND_ROTATE)

    def __init__(self, desc_ptr, flip):
        src = desc_ptr.contents
        self.keep = []
        d = ffi.SceneDesc()
        C.pointer(d)[0] = src          # every count and array as handed over ...
        d.flags = src.flags
        texs = [src.textures[i] for i in range(src.n_textures)]
        mats = []
        for i in range(src.n_materials):
            m = src.materials[i]
            if m.kind == ffi.VK_MAT_SPEC_DIFFUSE or m.kind == ffi.VK_MAT_DIELECTRIC:
                c = _solid_mix(src, i)
                if c is None:
                    raise ValueError(f"material {i}: a SpecDiffuse of non-solid textures has no emitter equivalent")
                texs.append(ffi.Texture(ffi.VK_TEX_SOLID, ffi.F3(*[float(v) for v in c]), 0, 0, 0.0))
                tex = len(texs) - 1
            elif m.kind == ffi.VK_MAT_DIFFUSE_LIGHT and src.textures[m.texture].kind == ffi.VK_TEX_SOLID:
                texs.append(ffi.Texture(ffi.VK_TEX_SOLID, ffi.F3(*[float(v) for v in _solid_mix(src, i)]), 0, 0, 0.0))
                tex = len(texs) - 1
            else:
                tex = m.texture
            mats.append(ffi.Material(ffi.VK_MAT_DIFFUSE_LIGHT, tex, 0.0, 0, 0))
        d.n_textures, d.textures = len(texs), self._arr(ffi.Texture, texs)
        d.n_materials, d.materials = len(mats), self._arr(ffi.Material, mats)
        if flip:
            fl = lambda r: r ^ ffi.VK_REF_FLIP if (r >> 28) in self.PRIM_KINDS else r
            bvh = [ffi.BvhNode(src.bvh[i].bb_min, src.bvh[i].bb_max, fl(src.bvh[i].left), fl(src.bvh[i].right)) for i in range(src.n_bvh)]
            d.bvh = self._arr(ffi.BvhNode, bvh)
            d.list_items = self._arr(C.c_uint32, [fl(src.list_items[i]) for i in range(src.n_list_items)])
            d.translates = self._arr(ffi.Translate, [ffi.Translate(fl(src.translates[i].child), src.translates[i].offset)
                                                     for i in range(src.n_translates)])
            d.rotates = self._arr(ffi.Rotate, [ffi.Rotate(fl(src.rotates[i].child), src.rotates[i].axis, src.rotates[i].sin_theta,
                                                          src.rotates[i].cos_theta) for i in range(src.n_rotates)])
            d.world = fl(src.world)
        self.desc = d
        self.ptr = C.pointer(d)

    def _arr(self, T, items):
        a = (T * max(1, len(items)))(*items)
        self.keep.append(a)
        return a


def ref_b_albedo(oracle, desc_ptr, cam, p):
    """per-sample albedo (spp, h, w, 3) of samples 0 .. p.samples_per_pixel - 1, from the oracle's own texture values"""
    out = None
    for flip in (False, True):
        sub = _Sub(desc_ptr, flip)
        q = ffi.RenderParams()
        C.pointer(q)[0] = p
        q.integrator, q.max_depth = ffi.VK_INTEGRATOR_SCATTER, 1
        if flip:                      # the background once: the copy as handed over sees it
            q.background, q.background_color = ffi.VK_BACKGROUND_SOLID, ffi.F3(0.0, 0.0, 0.0)
        _, ps = oracle.render_samples(sub.ptr, cam, q)
        rad = ps[:, :3].reshape(p.height, p.width, p.samples_per_pixel, 3).transpose(2, 0, 1, 3)
        out = rad.copy() if out is None else (out + rad).astype(f32)
    return out


# ---------------------------------------------------------------- aggregation
def aggregate(per_sample):
    """vk_render_aov's aggregation of single-sample results (dicts of (h, w[, 3]) arrays, in sample order): f32 sums in order, dropped
    samples (non-finite component) in n only"""
    n = len(per_sample)
    h, w = per_sample[0]["coverage"].shape
    sa, sn = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32)
    sd, hits = np.zeros((h, w), f32), np.zeros((h, w), np.uint32)
    for r in per_sample:
        hit = r["coverage"] == 1.0
        ok = np.isfinite(r["albedo"]).all(-1) & np.isfinite(r["normal"]).all(-1) & (~hit | np.isfinite(r["depth"]))
        # a single-sample call reports a dropped sample as coverage 0 and zero sums: what it adds below is then exactly nothing
        sa = np.where(ok[..., None], sa + r["albedo"], sa).astype(f32)
        sn = np.where(ok[..., None], sn + r["normal"], sn).astype(f32)
        sd = np.where(ok & hit, sd + r["depth"], sd).astype(f32)
        hits = hits + (ok & hit)
    fn = f32(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(hits > 0, sd / hits.astype(f32), f32(np.inf)).astype(f32)
    return dict(albedo=(sa / fn).astype(f32), normal=(sn / fn).astype(f32), depth=depth, coverage=(hits.astype(f32) / fn).astype(f32))
