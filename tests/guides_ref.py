"""Per-sample reference for the specular guides (vk_render_guides), built from the CPU oracle alone.  TESTS ONLY.

Segment 0 is oracle_first_hits (the radiance sample's own stream).  The continuation rule of include/vecchio_amd.h is restated here in
numpy float32, one operation at a time and unfused, in the reference's order (util.rs:14-23, material.rs:118-132,150-175), and every
continuation segment is oracle_hit(desc, p, dir, time, 0.001, inf, cseed) — BVHNode::hit on the scene as handed over, a medium drawing
from the stream the header names.  Albedo comes from oracle_texture_values through tests/aov_ref.py's rules.  +, -, *, /, sqrt and min
are correctly rounded in numpy as on the device, so the restatement is exact, not approximate.

oracle_hit does not say whether ConstantMedium::hit filled the record.  A medium's record has the phase function's material, so a hit
whose material is a phase function's and no primitive's is a medium hit; a scene that uses one material both ways is refused (none of
the test scenes does)."""
import numpy as np

import aov_ref
from vecchio_amd import ffi

f32 = np.float32
GOLDEN = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1
CHANNELS = ("albedo", "normal", "depth", "coverage", "bounces")


# ---------------------------------------------------------------- f32 vector arithmetic, in vk_trace.h's order
def v3(a):
    return np.asarray(a, dtype=f32).reshape(3)


def dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def length(d):
    return np.sqrt(dot(d, d), dtype=f32)


def unit(d):
    n = length(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (d / n).astype(f32)


def reflect(v, n):                                  # util.rs:14-16: v - n * dot(v, n) * 2
    return (v - ((n * dot(v, n)).astype(f32) * f32(2.0)).astype(f32)).astype(f32)


def refract(uv, n, eta):                            # util.rs:18-23
    cos_theta = -dot(uv, n)
    par = ((uv + (n * cos_theta).astype(f32)).astype(f32) * eta).astype(f32)
    with np.errstate(invalid="ignore"):
        perp = (n * -np.sqrt(f32(f32(1.0) - dot(par, par)), dtype=f32)).astype(f32)
    return (par + perp).astype(f32)


def fminf(a, b):
    """C fminf: the other argument when one is a NaN"""
    return b if np.isnan(a) else (a if np.isnan(b) else min(a, b))


def dielectric_direction(d, n, front, ir):
    """Dielectric::scatter's direction (material.rs:150-175) with the Schlick draw skipped; also whether it reflected"""
    ud = unit(d)
    ir = f32(ir)
    eta = f32(f32(1.0) / ir) if front else ir
    cos_theta = fminf(dot((-ud).astype(f32), n), f32(1.0))
    with np.errstate(invalid="ignore"):
        sin_theta = np.sqrt(f32(f32(1.0) - f32(cos_theta * cos_theta)), dtype=f32)
    if f32(eta * sin_theta) > f32(1.0):
        return reflect(ud, n), True
    return refract(ud, n, eta), False


def segment_seed(seed, pixel, sample, b):
    """cseed of continuation segment b (1..8) of (pixel, sample)"""
    return (int(seed) + GOLDEN * ((((int(pixel) << 32) | int(sample)) * 16 + int(b)) & MASK)) & MASK


# ---------------------------------------------------------------- the rule
def phase_materials(desc):
    media = {desc.media[i].material for i in range(desc.n_media)}
    prims = {desc.spheres[i].material for i in range(desc.n_spheres)}
    prims |= {desc.moving_spheres[i].material for i in range(desc.n_moving_spheres)}
    prims |= {desc.rects[i].material for i in range(desc.n_rects)}
    both = media & prims
    if both:
        raise ValueError(f"materials {sorted(both)} serve a medium and a primitive: oracle_hit cannot tell the two kinds of hit apart")
    return media


def is_delta(desc, mi, medium, fuzz_max):
    if medium:
        return False
    m = desc.materials[mi]
    return m.kind == ffi.VK_MAT_DIELECTRIC or (m.kind == ffi.VK_MAT_METAL and f32(m.param) <= f32(fuzz_max))


def _record(p, n, u, v, front, material):
    r = np.zeros(1, dtype=aov_ref_first_hit_dtype())
    r["p"], r["normal"], r["u"], r["v"], r["front"], r["material"] = p, n, u, v, int(front), material
    return r


def aov_ref_first_hit_dtype():
    import oracle_ffi
    return oracle_ffi.FIRST_HIT_DTYPE


def follow(oracle, desc_ptr, p, pixel, sample, rec, d, time, max_bounces, fuzz_max, phase):
    """one sample from its first hit `rec` (dict: p, normal, t, u, v, front, material, medium) along ray direction d: the terminal
    surface's (albedo, normal, depth, bounces) and the list of segments walked (for the closed-form self-tests)"""
    desc = desc_ptr.contents
    thr = np.ones(3, f32)
    ln = f32(0.0)
    b = 0
    d = v3(d)
    trail = []
    while True:
        n, pt = v3(rec["normal"]), v3(rec["p"])
        with np.errstate(over="ignore", invalid="ignore"):
            seg = f32(f32(rec["t"]) * length(d))
        mi = int(rec["material"])
        if not is_delta(desc, mi, rec["medium"], fuzz_max) or b >= max_bounces:
            a = aov_ref._albedo_a(oracle, desc_ptr, mi, _record(pt, n, rec["u"], rec["v"], rec["front"], mi))[0]
            normal = np.zeros(3, f32) if rec["medium"] else n
            with np.errstate(over="ignore", invalid="ignore"):
                return (thr * a).astype(f32), normal, f32(ln + seg), b, trail
        with np.errstate(over="ignore", invalid="ignore"):
            ln = f32(ln + seg)
        m = desc.materials[mi]
        if m.kind == ffi.VK_MAT_METAL:
            nd = reflect(unit(d), n)
            tint = oracle.texture_values(desc_ptr, m.texture, [rec["u"]], [rec["v"]], [pt])[0]
            with np.errstate(over="ignore", invalid="ignore"):
                thr = (thr * tint).astype(f32)
            how = "mirror"
        else:
            nd, tir = dielectric_direction(d, n, rec["front"], m.param)
            how = "tir" if tir else "refract"
        b += 1
        trail.append(dict(kind=how, origin=pt, direction=nd, normal=n))
        h = oracle.hit(desc_ptr, [float(x) for x in pt], [float(x) for x in nd], float(time), 0.001, float("inf"),
                       segment_seed(p.seed, pixel, sample, b))
        if h is None:
            with np.errstate(over="ignore", invalid="ignore"):
                return (thr * aov_ref.background(p, nd)).astype(f32), n, ln, b, trail
        d = nd
        rec = dict(p=v3(h["p"]), normal=v3(h["normal"]), t=f32(h["t"]), u=f32(h["u"]), v=f32(h["v"]), front=h["front"],
                   material=h["material"], medium=h["material"] in phase)


def ref_guides(oracle, desc_ptr, cam, p, samples, max_bounces=4, fuzz_max=0.0):
    """per sample of `samples` and pixel: dict of arrays — albedo, normal (n, h, w, 3), depth (inf on a primary miss), coverage, bounces
    (n, h, w); 'dropped' (a non-finite component: the sample adds to no sum); 'delta' (the first hit is a delta hit); 'first': reference
    (a) of tests/aov_ref.py for the same samples (what max_bounces = 0 gives)"""
    desc = desc_ptr.contents
    samples = list(samples)
    first = aov_ref.ref_a(oracle, desc_ptr, cam, p, samples)
    phase = phase_materials(desc)
    out = {ch: first[ch].copy() for ch in aov_ref.CHANNELS}
    out["bounces"] = np.zeros(first["coverage"].shape, f32)
    delta = np.zeros(first["coverage"].shape, bool)
    for k, s in enumerate(samples):
        fh = oracle.first_hits(desc_ptr, cam, p, s, 1)[:, :, 0]
        for y in range(p.height):
            for x in range(p.width):
                r = fh[y, x]
                if not r["hit"] or not is_delta(desc, int(r["material"]), bool(r["medium"]), fuzz_max):
                    continue
                delta[k, y, x] = True
                if max_bounces == 0:
                    continue
                rec = dict(p=r["p"], normal=r["normal"], t=r["t"], u=r["u"], v=r["v"], front=bool(r["front"]),
                           material=int(r["material"]), medium=False)
                a, n, dep, b, _ = follow(oracle, desc_ptr, p, y * p.width + x, s, rec, r["direction"], r["time"], max_bounces, fuzz_max,
                                         phase)
                out["albedo"][k, y, x], out["normal"][k, y, x], out["depth"][k, y, x], out["bounces"][k, y, x] = a, n, dep, b
    hit = out["coverage"] == 1
    ok = np.isfinite(out["albedo"]).all(-1) & np.isfinite(out["normal"]).all(-1) & (~hit | np.isfinite(out["depth"]))
    out["dropped"] = ~ok
    out["delta"] = delta
    out["first"] = first
    return out


def aggregate(per_sample):
    """vk_render_guides' aggregation of single-sample results: tests/aov_ref.py's for the four first-hit channels, and bounces = (the
    kept samples' counts, summed as integers) / (float)n — a dropped sample is reported with bounces 0"""
    out = aov_ref.aggregate(per_sample)
    sb = np.zeros(per_sample[0]["coverage"].shape, np.uint32)
    for r in per_sample:
        sb = sb + r["bounces"].astype(np.uint32)
    out["bounces"] = (sb.astype(f32) / f32(len(per_sample))).astype(f32)
    return out
