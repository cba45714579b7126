"""The replay for probe queries (vk_trace_probes), written from the contract in include/vecchio_amd.h.  TESTS ONLY; shared by the CPU and
the GPU test.

Sample s of probe i is "3 * tries draws for a uniform direction u, then ray_color(Ray{p, u, time}) on the same stream", and adds the 27 f32
products Y_k(u) * L_c to the probe's fixed-point sums.  The replay restates the first half in f32 numpy from the reference
(random_in_unit_sphere, util.rs:31-39; unit_vector) on the oracle's own gen_range(-1, 1) draws, the basis sh9 and the aggregation (with
tests/exact_sums.py's fixed-point conversion).  What it returns lets the second half be asked of the radiance query, which the existing
tests hold to the oracle: the ray (p, u, time, tmax) on the stream (ray_seed(seed, first_index + i), 0, s) resumed at counter 3 * tries."""
import numpy as np

import exact_sums
from irradiance_ref import assert_same_floats, assert_same_samples, bits, integrators_allowed, params_kwargs, scene  # noqa: F401
from rays_ref import ray_seed
from vecchio_amd.scene import KEY_DTYPE, RAY_DTYPE, make_probes, make_rays

f32 = np.float32
COEFFS = 9
# the coefficients of the basis as the header writes them
C0, C1, C2, C20, C22 = f32(0.282095), f32(0.488603), f32(1.092548), f32(0.315392), f32(0.546274)


def unit_sphere_point(draw3):
    """random_in_unit_sphere from a function that returns the stream's next 3 * m gen_range(-1, 1) draws: (point (3,) float32, tries)"""
    tries = 0
    while True:
        c = np.asarray(draw3(tries, 8), f32).reshape(-1, 3)
        l2 = f32(f32(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        ok = np.flatnonzero(~(l2 >= f32(1.0)))
        if len(ok):
            return c[ok[0]], tries + int(ok[0]) + 1
        tries += len(c)


def unit_vector(b):
    b = np.asarray(b, f32)
    l = np.sqrt(f32(f32(b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2]))
    with np.errstate(all="ignore"):
        return (b / l[..., None]).astype(f32)


def directions(oracle, probes, seed=0, first_index=0, samples_per_ray=1, first_sample=0, **_):
    """(dirs (n, samples_per_ray, 3) float32, keys (n, samples_per_ray) KEY_DTYPE: each sample's stream behind its direction's draws)"""
    probes = np.ascontiguousarray(probes, RAY_DTYPE).reshape(-1)
    n = len(probes)
    b = np.zeros((n, samples_per_ray, 3), f32)
    keys = np.zeros((n, samples_per_ray), KEY_DTYPE)
    for i in range(n):
        sd = ray_seed(seed, first_index + i)
        keys["seed"][i] = sd
        for k in range(samples_per_ray):
            # (the oracle's draws start at the stream's beginning: ask for the first 3 * (done + m) and keep the new ones)
            draw3 = lambda done, m: oracle.draws(sd, 0, first_sample + k, 1, 3 * (done + m), -1.0, 1.0)[3 * done:]
            b[i, k], tries = unit_sphere_point(draw3)
            keys["ctr"][i, k] = 3 * tries
    keys["sample"] = first_sample + np.arange(samples_per_ray, dtype=np.uint32)[None, :]
    return unit_vector(b), keys


def replayed_rays(probes, dirs):
    """one vk_ray per (probe, sample): the probe's position, time and tmax with the replayed direction; flat, probe-major"""
    probes = np.ascontiguousarray(probes, RAY_DTYPE).reshape(-1)
    spp = dirs.shape[1]
    return make_rays(np.repeat(probes["origin"], spp, 0), dirs.reshape(-1, 3), np.repeat(probes["time"], spp), np.repeat(probes["tmax"], spp))


def sh9(u):
    """the nine basis values of unit vectors (..., 3), in f32 in the header's form: (..., 9)"""
    u = np.asarray(u, f32)
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    with np.errstate(all="ignore"):
        Y = [np.broadcast_to(C0, x.shape), C1 * y, C1 * z, C1 * x, C2 * f32(x * y), C2 * f32(y * z),
             C20 * f32(f32(f32(3.0) * f32(z * z)) - f32(1.0)), C2 * f32(x * z), C22 * f32(f32(x * x) - f32(y * y))]
    return np.stack(Y, -1).astype(f32)


def exact_probes(samples, dirs):
    """(sh (n, 9, 3) float32, clamped samples, the integer sums (n, 9, 3)) that the hook's samples (n, spp, 4) and directions (n, spp, 4) must give: the products in
    f32, a sample with a non-finite component of L or u dropped, the fixed-point conversion of tests/exact_sums.py over a sample's 27
    products, integer sums, radiance_resolve_kernel's division"""
    samples, dirs = np.asarray(samples, f32), np.asarray(dirs, f32)
    n, spp = samples.shape[:2]
    L, u = samples[..., :3].reshape(-1, 3), dirs[..., :3].reshape(-1, 3)
    with np.errstate(all="ignore"):
        prod = (sh9(u)[:, :, None] * L[:, None, :]).astype(f32).reshape(-1, 27)
    keep = np.isfinite(L).all(1) & np.isfinite(u).all(1)
    clampv = exact_sums.accum_clamp_for(spp)
    fx = np.zeros((n * spp, 27), np.int64)
    with np.errstate(all="ignore"):
        fx[keep] = exact_sums.to_fixed(prod[keep], clampv)
        big = np.abs(prod[keep]).max(axis=1)
    clamped = int(((big > exact_sums.ACCUM_SMALL) & (big > clampv)).sum())
    sums = fx.reshape(n, spp, 27).sum(axis=1, dtype=np.int64)
    return exact_sums.resolve(sums, spp).reshape(n, COEFFS, 3), clamped, sums.reshape(n, COEFFS, 3)


# ---------------------------------------------------------------- the sky's closed form
SKY_K = np.array([0.5, 0.7, 1.0])


def sky_expected():
    """E[sh] (9, 3) under VK_BACKGROUND_SKY for a probe that sees nothing else: the sky is a_c + b_c * y with a_c = 1 + 0.5 (k_c - 1) and
    b_c = 0.5 (k_c - 1), so E[sh_0,c] = a_c * 0.282095, E[sh_1,c] = b_c * 0.488603 / 3 (E[y^2] = 1/3) and every other coefficient is 0"""
    a, b = 1.0 + 0.5 * (SKY_K - 1.0), 0.5 * (SKY_K - 1.0)
    want = np.zeros((COEFFS, 3))
    want[0] = a * 0.282095
    want[1] = b * 0.488603 / 3.0
    return want


def eval_band(n, mode, e):
    """how far vk_probe_eval can move when each of the 27 values moves by at most e: sum_k w_l(k) * |Y_k(unit(n))| * e"""
    n = np.asarray(n, np.float64)
    Y = np.abs(sh9(f32(n / np.linalg.norm(n))).astype(np.float64))
    w = np.full(9, 4 * np.pi) if mode == 0 else np.array([4 * np.pi] + [8 * np.pi / 3] * 3 + [np.pi] * 5)
    return float((w * Y).sum() * e)


def probes_in_box(n, lo, hi, t0=0.0, t1=0.0, rng_seed=11):
    """n probes at random positions of the box lo..hi, at random times of [t0, t1]; every third has a finite tmax — at or below
    VK_RAY_TMIN (no walk), short, long, NaN — and the directions hold arbitrary bytes (they are not read)"""
    rng = np.random.default_rng(rng_seed)
    pos = (f32(lo) + (f32(hi) - f32(lo)) * rng.uniform(0, 1, (n, 3))).astype(f32)
    pr = make_probes(pos, rng.uniform(t0, t1, n).astype(f32) if t1 > t0 else t0)
    pr["tmax"][::3] = np.resize(f32([0.001, 0.3, 25.0, np.nan, 0.004]), len(pr["tmax"][::3]))
    pr["direction"] = rng.normal(size=(n, 3)).astype(f32)
    pr["direction"][0] = np.nan
    return pr


def scene_box(oracle, desc, cam, p):
    """a box of positions inside the scene: the bounds of the first hits of a 20 x 12 pinhole frame, the camera's origin included"""
    from vecchio_amd import ffi
    pin = ffi.Camera.from_buffer_copy(cam)
    pin.lens_radius = 0.0
    q = ffi.RenderParams.from_buffer_copy(p)
    q.width, q.height, q.samples_per_pixel = 20, 12, 1
    fh = oracle.first_hits(desc, pin, q, 0, 1).reshape(-1)
    fh = fh[(fh["hit"] == 1) & np.isfinite(fh["p"]).all(1)]
    pts = np.concatenate([fh["p"], f32([list(cam.origin)])]) if len(fh) else f32([list(cam.origin)])
    lo, hi = np.clip(pts.min(0), -2000, 2000), np.clip(pts.max(0), -2000, 2000)
    return lo, np.maximum(hi, lo + f32(0.5))
