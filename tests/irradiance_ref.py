"""The direction replay for irradiance queries (vk_trace_irradiance).  TESTS ONLY; shared by the CPU and the GPU test.

Sample s of point i is "two draws for a cosine-weighted direction d around the normal, then ray_color(Ray{p, d, time}) on the same
stream".  The replay restates the first half in f32 numpy from the reference (random_cosine_direction, util.rs:52-63; ONB::new_from_w and
ONB::local, util.rs:95-110; Vec3::cross / unit_vector, vec3.rs:23-42), with the oracle's own primitives for what numpy cannot restate:
oracle.draws for r1 and r2, oracle.math(13 / 14) for the sine and cosine.  What it returns lets the second half be asked of the radiance
query, which the existing tests hold to the oracle: the ray (p, d, time, tmax) on the stream (ray_seed(seed, first_index + i), 0, s)
resumed at counter 2."""
import numpy as np

from rays_ref import ray_seed
from vecchio_amd.scene import KEY_DTYPE, RAY_DTYPE, make_rays

f32 = np.float32
PI_F = f32(3.14159265358979323846)


def _length2(a):
    return f32(f32(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def _unit(a):
    n = np.sqrt(_length2(a))
    return (a / n[..., None]).astype(f32)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(f32)


def onb_from_w(n):
    """(u, v, w) of ONB::new_from_w for normals (..., 3)"""
    w = _unit(np.asarray(n, f32))
    a = np.where((np.abs(w[..., 0]) > f32(0.9))[..., None], f32([0, 1, 0]), f32([1, 0, 0])).astype(f32)
    v = _unit(_cross(w, a))
    return _cross(w, v), v, w


def onb_local(uvw, a):
    u, v, w = uvw
    return ((u * a[..., 0:1] + v * a[..., 1:2]).astype(f32) + w * a[..., 2:3]).astype(f32)


def cosine_local(oracle, r1, r2):
    """random_cosine_direction from its two draws"""
    r1, r2 = np.asarray(r1, f32), np.asarray(r2, f32)
    z = np.sqrt(f32(1.0) - r2)
    phi = (f32(2.0) * r1) * PI_F
    s, c = oracle.math(13, phi).reshape(phi.shape), oracle.math(14, phi).reshape(phi.shape)
    return np.stack([c * np.sqrt(r2), s * np.sqrt(r2), z], -1).astype(f32)


def directions(oracle, points, seed=0, first_index=0, samples_per_ray=1, first_sample=0, **_):
    """(dirs (n, samples_per_ray, 3) float32, keys (n, samples_per_ray) KEY_DTYPE) for points (RAY_DTYPE: origin p, direction n)"""
    points = np.ascontiguousarray(points, RAY_DTYPE).reshape(-1)
    n = len(points)
    r = np.zeros((n, samples_per_ray, 2), f32)
    keys = np.zeros((n, samples_per_ray), KEY_DTYPE)
    for i in range(n):
        sd = ray_seed(seed, first_index + i)
        keys["seed"][i] = sd
        for k in range(samples_per_ray):
            r[i, k] = oracle.draws(sd, 0, first_sample + k, 0, 2)
    keys["sample"] = first_sample + np.arange(samples_per_ray, dtype=np.uint32)[None, :]
    keys["ctr"] = 2
    with np.errstate(all="ignore"):            # a zero or non-finite normal gives NaN axes, as in the reference
        uvw = onb_from_w(points["direction"])
        dirs = onb_local(tuple(x[:, None, :] for x in uvw), cosine_local(oracle, r[..., 0], r[..., 1]))
    return dirs, keys


def replayed_rays(points, dirs):
    """one vk_ray per (point, sample): the point's position, time and tmax with the replayed direction; flat, point-major"""
    points = np.ascontiguousarray(points, RAY_DTYPE).reshape(-1)
    spp = dirs.shape[1]
    return make_rays(np.repeat(points["origin"], spp, 0), dirs.reshape(-1, 3), np.repeat(points["time"], spp), np.repeat(points["tmax"], spp))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_floats(got, want, what=""):
    """bit for bit; a NaN equals a NaN whatever its payload"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0].tolist()}"


def assert_same_samples(got, want, what=""):
    """(.., 4) samples: rgb as assert_same_floats, the final counters equal"""
    assert_same_floats(got[..., :3], want[..., :3], what)
    np.testing.assert_array_equal(bits(got[..., 3]), bits(want[..., 3]), err_msg=f"{what}: final counters")


# ---------------------------------------------------------------- scenes and points the CPU and the GPU test share
def integrators_allowed(desc, default):
    """the scene's own integrator first, then the other one where vk_render would take it: the PDF integrator needs lights, the scatter
    integrator a world without SpecDiffuse"""
    from vecchio_amd import ffi
    d = desc.contents
    ok = {ffi.VK_INTEGRATOR_PDF: d.n_lights > 0,
          ffi.VK_INTEGRATOR_SCATTER: not any(d.materials[i].kind == ffi.VK_MAT_SPEC_DIFFUSE for i in range(d.n_materials))}
    return [default] + [i for i in ok if i != default and ok[i]]


def scene(kind, name, host_scenes):
    """(owner, desc, cam, p) of a scene of test_rays_emu.SCENES; the owner keeps the description's arrays alive (a radiance sample reads
    the texels of an image texture, which only the Desc that built the scene holds)"""
    import special_scenes
    import test_guides_emu as G
    import test_rays_emu as shared
    if kind == "special":
        return special_scenes.ALL[name]()
    if kind == "hand":
        return G.HAND_BUILT[name]()
    return (None,) + tuple(shared.scene(kind, name, host_scenes))


def params_kwargs(p, **over):
    """radiance parameters from render parameters"""
    kw = dict(seed=p.seed, first_index=0, samples_per_ray=1, first_sample=0, max_depth=p.max_depth, integrator=p.integrator,
              background=p.background, background_color=tuple(p.background_color))
    kw.update(over)
    return kw


def pixel_rays(cam, w, h):
    """the pixel-centre rays of a w x h frame through the camera's lens centre (RAY_DTYPE, row-major, time = the shutter's opening)"""
    o = f32(list(cam.origin))
    ys, xs = np.mgrid[0:h, 0:w]
    u, v = ((xs + 0.5) / w).astype(f32).reshape(-1, 1), ((ys + 0.5) / h).astype(f32).reshape(-1, 1)
    d = f32(list(cam.lower_left_corner)) + u * f32(list(cam.horizontal)) + v * f32(list(cam.vertical)) - o
    return make_rays(np.tile(o, (w * h, 1)), d.astype(f32), float(cam.time0))


def topped_up(points, n, lo, hi, t0, t1, rng_seed=7):
    """`points` cut to at most n - 33 and topped up to n with random positions in the box lo..hi and random normals that are not unit
    length — the first of them with |w.x| > 0.9, the second with |w.x| < 0.9 whatever the generator gives, so that both branches of
    ONB::new_from_w run"""
    rng = np.random.default_rng(rng_seed)
    keep = points[np.linspace(0, len(points) - 1, min(len(points), n - 33)).astype(int)] if len(points) else points[:0]
    k = n - len(keep)
    nrm = (rng.normal(size=(k, 3)) * rng.uniform(0.05, 40.0, (k, 1))).astype(f32)
    nrm[0] = f32([-7.5, 0.3, 0.2])
    nrm[1] = f32([0.1, -0.02, 3.0])
    pos = (f32(lo) + (f32(hi) - f32(lo)) * rng.uniform(0, 1, (k, 3))).astype(f32)
    extra = make_rays(pos, nrm, rng.uniform(t0, t1, k).astype(f32))
    out = np.concatenate([keep, extra])
    w = _unit(out["direction"])[:, 0]
    assert len(out) == n and (np.abs(w) > f32(0.9)).any() and (np.abs(w) < f32(0.9)).any()
    return out


def oracle_points(oracle, desc, cam, p, n=193):
    """n points: the first hits of a 20 x 12 pinhole frame (the hit point with the hit's normal, at the ray's time), topped up"""
    from vecchio_amd import ffi
    pin = ffi.Camera.from_buffer_copy(cam)
    pin.lens_radius = 0.0
    q = ffi.RenderParams.from_buffer_copy(p)
    q.width, q.height, q.samples_per_pixel = 20, 12, 1
    fh = oracle.first_hits(desc, pin, q, 0, 1).reshape(-1)
    fh = fh[(fh["hit"] == 1) & np.isfinite(fh["p"]).all(1) & np.isfinite(fh["normal"]).all(1)]
    pts = make_rays(fh["p"], fh["normal"], fh["time"])
    if len(fh):
        lo, hi = np.clip(fh["p"].min(0), -2000, 2000), np.clip(fh["p"].max(0), -2000, 2000)
    else:
        lo, hi = f32([-5, -5, -5]), f32([5, 5, 5])
    return topped_up(pts, n, lo, np.maximum(hi, lo + f32(0.5)), float(cam.time0), float(cam.time1))
