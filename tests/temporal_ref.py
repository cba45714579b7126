"""The temporal accumulator of include/vecchio_amd.h (vk_temporal_accumulate) restated in numpy, operation by operation in float32: every
array below is float32, every constant an np.float32, every expression parenthesised as the header writes it, so that numpy's correctly
rounded + - * / and sqrt reproduce the device's bits.  Written from the header's definition with whole-image arrays and gathers, not from
the kernel: a tap is a gathered copy of the history, a skipped tap adds nothing (np.where), fmaxf / fminf are np.fmax / np.fmin.

    acc = Accumulator(width, height, max_history=32, depth_tol=0.02, normal_cos_min=0.9, albedo_floor=1e-3)
    out_color, out_stderr3, out_history = acc.accumulate(cam, color, stderr3, albedo, normal, depth)

Images are (height, width, 3) float32 (depth and out_history (height, width)), row 0 the bottom row; stderr3 and albedo may be None.
A camera is anything with the fields of vk_camera (origin, lower_left_corner, horizontal, vertical, w): an ffi.Camera or camera() below.
acc.took is the mask of the pixels of the last frame that took the history branch (vk_temporal_info.pixels_with_history counts them);
acc.proj = (px, py, ok) are the last frame's reprojected coordinates."""
import types

import numpy as np

f32 = np.float32
INF = f32(np.inf)
DEFAULTS = dict(max_history=32, depth_tol=0.02, normal_cos_min=0.9, albedo_floor=1e-3)


def vec(v):
    return np.array([v[0], v[1], v[2]], f32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def first_hit_dirs(cam, width, height):
    """d of the header: the pixel centres through the lens centre, (height, width, 3)"""
    ys, xs = np.mgrid[0:height, 0:width]
    s = ((xs.astype(f32) + f32(0.5)) / f32(width - 1))[..., None]
    t = ((ys.astype(f32) + f32(0.5)) / f32(height - 1))[..., None]
    return ((vec(cam.lower_left_corner) + vec(cam.horizontal) * s) + vec(cam.vertical) * t) - vec(cam.origin)


def project(e, prev, width, height):
    """a point e (relative to the previous camera's origin) -> (px, py, ok) in the previous frame's pixel coordinates"""
    o, H, V, w = vec(prev.origin), vec(prev.horizontal), vec(prev.vertical), vec(prev.w)
    q = vec(prev.lower_left_corner) - o
    fw = -dot(q, w)
    ew = -dot(e, w)
    with np.errstate(all="ignore"):
        g = e * (fw / ew)[..., None] - q
        px = (dot(g, H) / dot(H, H)) * f32(width - 1) - f32(0.5)
        py = (dot(g, V) / dot(V, V)) * f32(height - 1) - f32(0.5)
        ok = (ew > 0) & (px > f32(-1)) & (px < f32(width)) & (py > f32(-1)) & (py < f32(height))
    return px, py, ok


class Accumulator:
    def __init__(self, width, height, max_history=32, depth_tol=0.02, normal_cos_min=0.9, albedo_floor=1e-3):
        self.w, self.h = width, height
        self.max_history, self.depth_tol, self.normal_cos_min, self.albedo_floor = f32(max_history), f32(depth_tol), f32(normal_cos_min), f32(albedo_floor)
        self.reset()

    def reset(self):
        self.hist = None          # (I, V, N, n, z, cam) of the previous frame
        self.took = None
        self.proj = None

    def accumulate(self, cam, color, stderr3, albedo, normal, depth):
        h, w = self.h, self.w
        color = np.ascontiguousarray(color, f32)
        with np.errstate(all="ignore"):
            a = np.fmax(albedo, self.albedo_floor) if albedo is not None else np.ones((h, w, 3), f32)
            valid = np.isfinite(color).all(-1)
            I = color / a
            if stderr3 is not None:
                valid &= np.isfinite(stderr3).all(-1)
                S = stderr3 / a
                Vc = S * S
            else:
                Vc = np.zeros((h, w, 3), f32)
            l2 = dot(normal, normal)
            has_n = ~(l2 < f32(1e-12)) & np.isfinite(l2)
            n = np.zeros((h, w, 3), f32)
            n[has_n] = normal[has_n] / np.sqrt(l2[has_n])[:, None]
            z = np.where(np.isfinite(depth), depth, INF).astype(f32)
            miss = np.isinf(z)

            Iout, Vout, N = I, Vc, np.ones((h, w), f32)
            took = np.zeros((h, w), bool)
            if self.hist is not None:
                Ip, Vp, Np, np_, zp, prev = self.hist
                d = first_hit_dirs(cam, w, h)
                length = np.sqrt(dot(d, d))
                e_hit = (vec(cam.origin) + d * (z / length)[..., None]) - vec(prev.origin)
                e = np.where(miss[..., None], d, e_hit).astype(f32)
                px, py, ok = project(e, prev, w, h)
                self.proj = (px, py, ok)
                ze = np.sqrt(dot(e, e))
                xf, yf = np.floor(px), np.floor(py)
                fx, fy = px - xf, py - yf
                x0 = np.where(ok, xf, 0).astype(np.int64)
                y0 = np.where(ok, yf, 0).astype(np.int64)
                W, M = np.zeros((h, w), f32), np.zeros((h, w), f32)
                J, U = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32)
                for k in range(4):
                    qx, qy = x0 + (k & 1), y0 + (k >> 1)
                    b = (fx if k & 1 else f32(1) - fx) * (fy if k >> 1 else f32(1) - fy)
                    inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    gx, gy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    Iq, Vq, Nq, nq, zq = Ip[gy, gx], Vp[gy, gx], Np[gy, gx], np_[gy, gx], zp[gy, gx]
                    c_z = np.where(miss, np.isposinf(zq), np.abs(zq - ze) <= self.depth_tol * ze)
                    flat_p, flat_q = ~has_n, (nq == 0).all(-1)
                    c_n = np.where(flat_p | flat_q, flat_p & flat_q, dot(n, nq) >= self.normal_cos_min)
                    good = inside & (Nq > 0) & c_z & c_n
                    W = np.where(good, W + b, W)
                    J = np.where(good[..., None], J + b[..., None] * Iq, J)
                    U = np.where(good[..., None], U + b[..., None] * Vq, U)
                    M = np.where(good, M + b * Nq, M)
                took = valid & ok & (W >= f32(0.01))
                Nb = np.fmin(M / W + f32(1), self.max_history)
                alpha = f32(1) / Nb
                k1 = f32(1) - alpha
                Ib = k1[..., None] * (J / W[..., None]) + alpha[..., None] * I
                Vb = (k1 * k1)[..., None] * (U / W[..., None]) + (alpha * alpha)[..., None] * Vc
                Iout = np.where(took[..., None], Ib, I).astype(f32)
                Vout = np.where(took[..., None], Vb, Vc).astype(f32)
                N = np.where(took, Nb, f32(1)).astype(f32)
            N = np.where(valid, N, f32(0)).astype(f32)
            out_color = np.where(valid[..., None], Iout * a, color).astype(f32)
            out_stderr3 = None
            if stderr3 is not None:
                out_stderr3 = np.where(valid[..., None], np.sqrt(Vout) * a, stderr3).astype(f32)
        self.took = took
        self.hist = (Iout.astype(f32), Vout.astype(f32), N, n, z, snapshot(cam))
        return out_color, out_stderr3, N.copy()


def snapshot(cam):
    return types.SimpleNamespace(origin=vec(cam.origin), lower_left_corner=vec(cam.lower_left_corner), horizontal=vec(cam.horizontal),
                                 vertical=vec(cam.vertical), w=vec(cam.w))


# ---- cameras and synthetic frame sequences (tests/test_temporal_abi.py, tests/test_gpu_temporal.py)
def camera(look_from, look_at, vfov_deg=40.0, aspect=16.0 / 9.0, vup=(0.0, 1.0, 0.0)):
    """a pinhole camera with the fields of vk_camera (the construction of Camera::new with focus distance 1), in float32"""
    lf, la, up = np.array(look_from, np.float64), np.array(look_at, np.float64), np.array(vup, np.float64)
    vh = 2.0 * np.tan(np.radians(vfov_deg) / 2.0)
    vw = aspect * vh
    w = (lf - la) / np.linalg.norm(lf - la)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    H, V = vw * u, vh * v
    return types.SimpleNamespace(origin=vec(lf), lower_left_corner=vec(lf - H / 2 - V / 2 - w), horizontal=vec(H), vertical=vec(V),
                                 u=vec(u), v=vec(v), w=vec(w), lens_radius=f32(0), time0=f32(0), time1=f32(1))


def orbit(angle_deg, radius=13.0, height=2.0, **kw):
    """a camera on a circle around the y axis looking at the origin (the RotatingCamera of scene.rs:48-91 in spirit)"""
    a = np.radians(angle_deg)
    return camera((radius * np.sin(a), height, radius * np.cos(a)), (0.0, 0.5, 0.0), **kw)


SPHERES = (((0.0, 1.0, 0.0), 1.0), ((-3.0, 0.7, 1.5), 0.7), ((2.5, 0.5, 2.0), 0.5), ((1.0, 0.3, 4.0), 0.3))


def frame(cam, width, height, rng, invalid=True):
    """the ground plane y = 0 and SPHERES seen through the pixel centres of `cam`: noisy colour, standard error, albedo, normal, depth"""
    d = first_hit_dirs(cam, width, height).astype(np.float64)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.array(cam.origin, np.float64)
    with np.errstate(all="ignore"):
        t = np.where(d[..., 1] < -1e-9, -o[1] / d[..., 1], np.inf)
        t = np.where(t < 60.0, t, np.inf)                               # the plane ends: sky beyond
        nrm = np.zeros((height, width, 3))
        nrm[np.isfinite(t)] = (0.0, 1.0, 0.0)
        which = np.where(np.isfinite(t), 0, -1)
        for i, (c, r) in enumerate(SPHERES):
            oc = o - np.array(c)
            bq = (d * oc).sum(-1)
            disc = bq * bq - ((oc * oc).sum() - r * r)
            ts = np.where(disc > 0, -bq - np.sqrt(np.abs(disc)), np.inf)
            hit = (ts > 1e-3) & (ts < t)
            t = np.where(hit, ts, t)
            nrm[hit] = ((o + d * ts[..., None] - np.array(c)) / r)[hit]
            which = np.where(hit, i + 1, which)
    pos = o + d * np.where(np.isfinite(t), t, 0.0)[..., None]
    checker = ((np.floor(pos[..., 0]) + np.floor(pos[..., 2])) % 2 == 0)
    albedo = np.where(checker[..., None], (0.8, 0.3, 0.2), (0.2, 0.6, 0.9))
    palette = np.array([(0.5, 0.7, 1.0), (0, 0, 0), (0.7, 0.7, 0.1), (0.0, 0.0, 0.0), (0.9, 0.9, 0.9), (0.3, 0.8, 0.3)])
    albedo = np.where((which == 0)[..., None], albedo, palette[which + 1])          # (sphere 2 has an albedo below the floor)
    shade = 0.3 + 0.7 * np.clip(nrm @ np.array([0.3, 0.8, 0.5]), 0, 1)
    sigma = f32(0.08)
    color = ((albedo * shade[..., None]).astype(f32) + sigma * rng.standard_normal((height, width, 3)).astype(f32)).astype(f32)
    stderr3 = (sigma * (f32(0.5) + rng.random((height, width, 3)).astype(f32))).astype(f32)
    normal = (nrm.astype(f32) * f32(0.8)).astype(f32)                  # averaged: not unit length
    normal[which == 4] = f32(0)                                        # a medium: hit, no normal
    depth = np.where(np.isfinite(t), t, np.inf).astype(f32)
    if invalid and width * height >= 12:
        for k in range(max(1, width * height // 97)):
            y, x = int(rng.integers(height)), int(rng.integers(width))
            if k % 3 == 0:
                color[y, x, k % 3] = np.nan
            elif k % 3 == 1:
                color[y, x, 1] = INF
            else:
                stderr3[y, x, 2] = np.nan
    return dict(color=color, stderr3=stderr3, albedo=albedo.astype(f32), normal=normal, depth=depth)


def synthetic(width, height, seed=0, frames=2, step_deg=0.5, invalid=True, turn_away=False):
    """[(camera, frame), ...]: `frames` views of the same static scene from an orbiting camera, step_deg apart (turn_away: the last camera
    looks the other way, so that nothing of it was seen before)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(frames):
        cam = orbit(20.0 + step_deg * i, aspect=width / height)
        if turn_away and i == frames - 1:
            cam = camera(cam.origin, 2.0 * np.array(cam.origin, np.float64) - np.array((0.0, 0.5, 0.0)), aspect=width / height)
        out.append((cam, frame(cam, width, height, rng, invalid)))
    return out


def to_ffi(cam):
    from vecchio_amd import ffi
    c = ffi.Camera()
    for k in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w"):
        setattr(c, k, ffi.F3(*[float(x) for x in getattr(cam, k)]))
    c.lens_radius, c.time0, c.time1 = float(cam.lens_radius), float(cam.time0), float(cam.time1)
    return c
