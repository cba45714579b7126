"""What tests/test_shade_emu.py and tests/test_gpu_shade.py share: the scene set (test_rays_emu's, split by media), the census of what
the media-free scenes contain, the ray set, the integrators vk_render allows on a scene, and the bit-for-bit comparisons."""
import numpy as np

import irradiance_ref
import special_scenes
import test_rays_emu as R
from descs import Desc, camera, params
from vecchio_amd import ffi
from vecchio_amd.scene import SHADED_DTYPE

f32 = np.float32
W, H = 16, 12
SEED, FIRST = 0xC0FFEE12345, 7
DEPTHS = (8, 50)


def everything_lit():
    """A hand-built scene without media that holds every kind the shading code branches on: Lambertian, Metal, Dielectric, DiffuseLight
    and SpecDiffuse (nested once) materials; Solid, Checker, Image and Noise textures; a Rect light and a Sphere light (the sphere inside
    a list, as Vec::random meets it)."""
    d = Desc()
    rng = np.random.default_rng(5)
    img = d.image(rng.integers(0, 256, (7, 5, 3)).astype(np.uint8))
    chk = d.checker(d.solid(0.1, 0.2, 0.3), img)
    marble = d.noise(4.0, seed=2)
    lam_img = d.mat(ffi.VK_MAT_LAMBERTIAN, img)
    lam_chk = d.mat(ffi.VK_MAT_LAMBERTIAN, chk)
    lam_noise = d.mat(ffi.VK_MAT_LAMBERTIAN, marble)
    metal = d.mat(ffi.VK_MAT_METAL, d.solid(0.8, 0.7, 0.6), 0.2)
    metal_noise = d.mat(ffi.VK_MAT_METAL, marble, 0.0)
    glass = d.mat(ffi.VK_MAT_DIELECTRIC, 0, 1.5)
    inner = d.mat(ffi.VK_MAT_SPEC_DIFFUSE, 0, 0.5, metal_noise, lam_chk)
    spec = d.mat(ffi.VK_MAT_SPEC_DIFFUSE, 0, 0.3, metal, inner)
    lamp = d.light(7.0, 6.0, 5.0)
    bulb = d.mat(ffi.VK_MAT_DIFFUSE_LIGHT, chk)
    panel = d.xz_rect(-1.5, 1.5, -1.5, 1.5, 3.9, lamp)
    ball = d.sphere((2.6, 2.4, -1.0), 0.5, bulb)
    objs = [d.flip(panel), ball,
            d.xz_rect(-6, 6, -6, 6, -1.0, lam_chk), d.xy_rect(-6, 6, -1, 4, -4.0, lam_img), d.yz_rect(-1, 4, -6, 6, -4.0, spec),
            d.sphere((-1.6, 0.0, 0.0), 1.0, glass), d.sphere((0.9, 0.0, -0.5), 1.0, lam_noise), d.sphere((0.2, -0.5, 1.8), 0.5, metal),
            d.sphere((2.4, -0.3, 1.0), 0.7, spec)]
    world = special_scenes._bvh_chain(d, objs)
    desc = d.finish(world, lights=[panel, d.list_([ball])])
    return d, desc, camera((0.5, 1.5, 8.0), (0, 0.8, 0), vfov=45.0, aspect=W / H), \
        params(W, H, 1, seed=9, integrator=ffi.VK_INTEGRATOR_PDF, background=ffi.VK_BACKGROUND_SOLID, bg=(0.02, 0.03, 0.05))


_OWN = {}


def scene(kind, name, host_scenes):
    """(desc, cam, p): test_rays_emu's scenes, and this module's own.  What built a hand-made description owns its arrays — an image
    texture's texels among them, which shading reads — and is kept here for as long as the tests run."""
    import test_guides_emu as G
    if kind in ("shade", "special", "hand"):
        if (kind, name) not in _OWN:
            make = everything_lit if kind == "shade" else (special_scenes.ALL[name] if kind == "special" else G.HAND_BUILT[name])
            d, desc, cam, p = make()
            if kind == "special":
                p.width, p.height = G.W, G.H
            _OWN[(kind, name)] = (d, desc, cam, p)
        return _OWN[(kind, name)][1:]
    return R.scene(kind, name, host_scenes)


ALL_SCENES = list(R.SCENES) + [("shade", "everything_lit")]


def split_by_media(host_scenes):
    """(media-free scenes, scenes with a ConstantMedium)"""
    plain, media = [], []
    for kind, name in ALL_SCENES:
        desc, _, _ = scene(kind, name, host_scenes)
        (media if desc.contents.n_media else plain).append((kind, name))
    return plain, media


def census(desc):
    """(material kinds, texture kinds reachable from a material, kinds of the objects the lights list samples) of a description"""
    d = desc.contents
    mats = {int(d.materials[i].kind) for i in range(d.n_materials)}
    texs = set()

    def walk(t, depth=0):
        k = int(d.textures[t].kind)
        texs.add(k)
        if k == ffi.VK_TEX_CHECKER and depth < 16:
            walk(d.textures[t].a, depth + 1)
            walk(d.textures[t].b, depth + 1)

    for i in range(d.n_materials):
        if d.materials[i].kind in (ffi.VK_MAT_LAMBERTIAN, ffi.VK_MAT_METAL, ffi.VK_MAT_DIFFUSE_LIGHT, ffi.VK_MAT_ISOTROPIC):
            walk(d.materials[i].texture)
    lights = set()
    for i in range(d.n_lights):
        ref = int(d.lights[i])
        if ref & ffi.VK_REF_FLIP:
            continue                               # (FlipFace forwards neither pdf_value nor random)
        if ref >> 28 == ffi.VK_KIND_LIST:
            l = d.lists[ref & ffi.VK_REF_INDEX_MASK]
            for j in range(l.count):
                r = int(d.list_items[l.first + j])
                if not r & ffi.VK_REF_FLIP:
                    lights.add(r >> 28)
        else:
            lights.add(ref >> 28)
    return mats, texs, lights


def integrators(desc):
    """the integrators vk_render allows on the scene"""
    d = desc.contents
    out = []
    if d.n_lights:
        out.append(ffi.VK_INTEGRATOR_PDF)
    if not any(d.materials[i].kind == ffi.VK_MAT_SPEC_DIFFUSE for i in range(d.n_materials)):
        out.append(ffi.VK_INTEGRATOR_SCATTER)
    return out


def rays_of(cam):
    """the pixel-centre primary rays of a W x H frame, then six more: finite tmax (short of everything, and generous), tmax at and below
    VK_RAY_TMIN, and a NaN direction"""
    prim = irradiance_ref.pixel_rays(cam, W, H)
    extra = prim[[5, W * H // 2 + 3, W * H // 2 + 4, 17, 40, W * H - 9]].copy()
    extra["tmax"] = f32([1e-2, 1e4, 3.0, ffi.VK_RAY_TMIN, -1.0, np.inf])
    extra["direction"][5, 1] = np.nan
    return np.concatenate([prim, extra])


def shade_kwargs(p, integrator, max_depth):
    return dict(max_depth=max_depth, integrator=integrator, background=p.background, background_color=tuple(p.background_color))


def radiance_kwargs(p, integrator, max_depth, **over):
    kw = dict(seed=SEED, first_index=FIRST, samples_per_ray=1, first_sample=0, **shade_kwargs(p, integrator, max_depth))
    kw.update(over)
    return kw


def assert_samples_equal(got, want, what=""):
    """(n, 4) float32 rows — rgb and the counter's bit pattern — bit for bit; a NaN equals a NaN whatever its payload"""
    g, w = np.ascontiguousarray(got, f32).view(np.uint32), np.ascontiguousarray(want, f32).view(np.uint32)
    assert g.shape == w.shape, (g.shape, w.shape)
    both_nan = np.zeros(g.shape, bool)
    both_nan[:, :3] = np.isnan(got[:, :3]) & np.isnan(want[:, :3])
    bad = (g != w) & ~both_nan
    if bad.any():
        i = int(np.argwhere(bad.any(1))[0, 0])
        raise AssertionError(f"{what}: {int(bad.any(1).sum())} of {len(g)} samples differ; first {i}: got {got[i]} ctr {g[i, 3]}, "
                             f"want {want[i]} ctr {w[i, 3]}")


# words of vk_shaded that hold floats: next (0..7), state.thr (8..10), state.acc (12..14)
_FLOAT_WORDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14]


def assert_shaded_equal(got, want, what=""):
    """SHADED_DTYPE arrays on all 96 bytes; a NaN equals a NaN whatever its payload"""
    g = np.ascontiguousarray(got, SHADED_DTYPE).view(np.uint32).reshape(-1, 24)
    w = np.ascontiguousarray(want, SHADED_DTYPE).view(np.uint32).reshape(-1, 24)
    assert g.shape == w.shape, (g.shape, w.shape)
    both_nan = np.zeros(g.shape, bool)
    both_nan[:, _FLOAT_WORDS] = np.isnan(g.view(f32)[:, _FLOAT_WORDS]) & np.isnan(w.view(f32)[:, _FLOAT_WORDS])
    bad = (g != w) & ~both_nan
    if bad.any():
        i = int(np.argwhere(bad.any(1))[0, 0])
        raise AssertionError(f"{what}: {int(bad.any(1).sum())} of {len(g)} items differ; first {i}:\n  got  {got[i]}\n  want {want[i]}")


STATUSES = (ffi.VK_SHADE_MISS, ffi.VK_SHADE_SCATTERED, ffi.VK_SHADE_ENDED, ffi.VK_SHADE_BAD_HIT)
