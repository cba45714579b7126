"""The denoiser of include/vecchio_amd.h (vk_denoise) restated in numpy, operation by operation in float32: every array below is float32,
every constant an np.float32, every expression parenthesised as the header writes it, so that numpy's correctly rounded + - * / and
sqrt reproduce the device's bits.  Written from the header's definition with whole-image shifts, not from the kernel: a tap is a shifted
copy of the image, a skipped tap adds nothing (np.where), fmaxf is np.fmax (it drops a NaN).

    denoise(color, stderr3, albedo, normal, depth, levels=5, normal_squarings=7, sigma_l=4, sigma_z=1, albedo_floor=1e-3) -> out

Images are (height, width, 3) float32 (depth (height, width)), row 0 the bottom row; any guide may be None.  `trace=True` also returns
the per-level (I, V) images."""
import numpy as np

f32 = np.float32
INF = f32(np.inf)
K = (f32(0.375), f32(0.25), f32(0.0625))
DEFAULTS = dict(levels=5, normal_squarings=7, sigma_l=4.0, sigma_z=1.0, albedo_floor=1e-3)


def falloff(x):
    """E(x) = max(0, 1 - x/8)^8 by three squarings"""
    t = np.fmax(f32(0), f32(1) - x * f32(0.125))
    t = t * t
    t = t * t
    return t * t


def lum(c):
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


def shifted(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside the image"""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = slice(max(dy, 0), min(h + dy, h)), slice(max(-dy, 0), min(h - dy, h))
    xs, xd = slice(max(dx, 0), min(w + dx, w)), slice(max(-dx, 0), min(w - dx, w))
    if ys.start < ys.stop and xs.start < xs.stop:
        b[yd, xd] = a[ys, xs]
    return b


def prepare(color, stderr3, albedo, normal, depth, albedo_floor):
    h, w = color.shape[:2]
    a = np.fmax(albedo, f32(albedo_floor)) if albedo is not None else np.ones((h, w, 3), f32)
    valid = np.isfinite(color).all(-1)
    I = color / a
    if stderr3 is not None:
        valid &= np.isfinite(stderr3).all(-1)
        sd = lum(stderr3 / a)
        V = sd * sd
    else:
        V = np.zeros((h, w), f32)
    n = np.zeros((h, w, 3), f32)
    if normal is not None:
        l2 = (normal[..., 0] * normal[..., 0] + normal[..., 1] * normal[..., 1]) + normal[..., 2] * normal[..., 2]
        has = ~(l2 < f32(1e-12)) & np.isfinite(l2)
        n[has] = normal[has] / np.sqrt(l2[has])[:, None]
    z = np.full((h, w), INF, f32)
    g = np.zeros((h, w, 2), f32)
    if depth is not None:
        z = np.where(np.isfinite(depth), depth, INF).astype(f32)
        fin = np.isfinite(z)
        for axis, (dx, dy) in enumerate(((1, 0), (0, 1))):
            zp, zm = shifted(z, dx, dy, INF), shifted(z, -dx, -dy, INF)         # z(x+1), z(x-1): +inf outside the image
            fp, fm = np.isfinite(zp), np.isfinite(zm)
            both = (zp - zm) * f32(0.5)
            g[..., axis] = np.where(fin, np.where(fp & fm, both, np.where(fp, zp - z, np.where(fm, z - zm, f32(0)))), f32(0))
    return a, valid, I.astype(f32), V.astype(f32), n, z, g


def level(I, V, valid, n, z, g, s, have_l, have_n, have_z, normal_squarings, sigma_l, sigma_z):
    h, w = V.shape
    Y = lum(I)
    den_l = None
    if have_l:
        acc, ws = np.zeros((h, w), f32), np.zeros((h, w), f32)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = shifted(valid, dx, dy, False)
                kw = f32((2 if dx == 0 else 1) * (2 if dy == 0 else 1))
                Vq = shifted(V, dx, dy, f32(0))
                acc = np.where(ok, acc + kw * Vq, acc)
                ws = np.where(ok, ws + kw, ws)
        with np.errstate(all="ignore"):
            den_l = f32(sigma_l) * np.sqrt(acc / ws) + f32(1e-6)
    no_n = (n == 0).all(-1)
    far = np.isinf(z)
    W, U, J = np.zeros((h, w), f32), np.zeros((h, w), f32), np.zeros((h, w, 3), f32)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                hk = K[abs(dx)] * K[abs(dy)]
                if dx == 0 and dy == 0:
                    wgt, ok, Iq, Vq = np.full((h, w), hk, f32), np.ones((h, w), bool), I, V
                else:
                    ox, oy = s * dx, s * dy
                    ok = shifted(valid, ox, oy, False)
                    Iq, Vq = shifted(I, ox, oy, f32(0)), shifted(V, ox, oy, f32(0))
                    wn = np.ones((h, w), f32)
                    if have_n:
                        nq, no_q = shifted(n, ox, oy, f32(0)), shifted(no_n, ox, oy, True)
                        c = np.fmax(f32(0), (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
                        for _ in range(normal_squarings):
                            c = c * c
                        wn = np.where(no_n & no_q, f32(1), np.where(no_n | no_q, f32(0), c)).astype(f32)
                    xz = np.zeros((h, w), f32)
                    if have_z:
                        zq = shifted(z, ox, oy, INF)
                        far_q = np.isinf(zq)
                        ok = ok & (far == far_q)                                  # one of the two at +inf: the tap is skipped
                        den = f32(sigma_z) * (np.abs(g[..., 0] * f32(ox) + g[..., 1] * f32(oy)) + f32(0.001) * z)
                        xz = np.where(far, f32(0), np.abs(z - zq) / den).astype(f32)
                    xl = np.zeros((h, w), f32)
                    if have_l:
                        xl = np.abs(Y - lum(Iq)) / den_l
                    wgt = ((hk * wn) * falloff(xz)) * falloff(xl)
                W = np.where(ok, W + wgt, W)
                J = np.where(ok[..., None], J + wgt[..., None] * Iq, J)
                U = np.where(ok, U + (wgt * wgt) * Vq, U)
        I2, V2 = J / W[..., None], U / (W * W)
    return np.where(valid[..., None], I2, I).astype(f32), np.where(valid, V2, V).astype(f32)


def denoise(color, stderr3=None, albedo=None, normal=None, depth=None, levels=5, normal_squarings=7, sigma_l=4.0, sigma_z=1.0,
            albedo_floor=1e-3, trace=False):
    color = np.ascontiguousarray(color, f32)
    with np.errstate(all="ignore"):
        a, valid, I, V, n, z, g = prepare(color, stderr3, albedo, normal, depth, albedo_floor)
        steps = []
        for i in range(levels):
            I, V = level(I, V, valid, n, z, g, 1 << i, stderr3 is not None, normal is not None, depth is not None, normal_squarings,
                         sigma_l, sigma_z)
            steps.append((I, V))
        out = np.where(valid[..., None], I * a, color).astype(f32)
    return (out, steps) if trace else out


# ---- synthetic inputs with edges, +inf depths, zero normals and invalid pixels (tests/test_gpu_denoise.py, tools/denoise_report.py)
def synthetic(width, height, seed=0, invalid=True):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:height, 0:width]
    left = xs < width // 2
    top = ys >= (2 * height) // 3
    albedo = np.where(((xs // 5 + ys // 3) % 2 == 0)[..., None], f32([0.8, 0.3, 0.2]), f32([0.2, 0.6, 0.9])).astype(f32)
    albedo[top] = f32(0)                                                # below the floor
    base = np.where(left[..., None], f32([0.9, 0.7, 0.5]), f32([0.1, 0.2, 0.4])).astype(f32)
    sigma = f32(0.08)
    color = (albedo * base + sigma * rng.standard_normal((height, width, 3)).astype(f32)).astype(f32)
    stderr3 = (sigma * (f32(0.5) + rng.random((height, width, 3)).astype(f32))).astype(f32)
    normal = np.where(left[..., None], f32([0.0, 0.6, 0.8]), f32([1.0, 0.0, 0.0])).astype(f32)
    normal = (normal * f32(0.7) + f32(0.02) * rng.standard_normal((height, width, 3)).astype(f32)).astype(f32)   # averaged: not unit length
    depth = (f32(5) + f32(0.03) * xs + f32(0.05) * ys + np.where(left, f32(0), f32(3))).astype(f32)
    sky = (ys >= height - max(1, height // 5)) & (xs % 7 != 0)
    depth[sky] = INF
    normal[sky] = f32(0)
    if invalid and width * height >= 12:
        for k in range(max(1, width * height // 97)):
            y, x = int(rng.integers(height)), int(rng.integers(width))
            if k % 3 == 0:
                color[y, x, k % 3] = np.nan
            elif k % 3 == 1:
                color[y, x, 1] = INF
            else:
                stderr3[y, x, 2] = np.nan
    return dict(color=color, stderr3=stderr3, albedo=albedo, normal=normal, depth=depth)
