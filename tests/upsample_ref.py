"""Guided upsampling (vk_upsample_*) restated in vectorised numpy, f32 throughout, in the order include/vecchio_amd.h ("guided upsampling")
writes down: one sweep over the 16 taps, ty the outer loop and tx the inner, every high pixel at once.  The kernels, the host build
(tests/emu/emu_upsample.cpp) and this file agree bit for bit, a NaN's payload aside.  TESTS ONLY."""
import numpy as np

f32 = np.float32
F = lambda v: np.float32(v)


def ratios(lo, hi):
    """(r, s) of one axis: (float)((double)(lo - 1) / (double)(hi - 1)) and its inverse"""
    return f32(np.float64(lo - 1) / np.float64(hi - 1)), f32(np.float64(hi - 1) / np.float64(lo - 1))


def centres(n_hi, r):
    """px of every high pixel of one axis: ((float)X + 0.5f) * r - 0.5f"""
    X = np.arange(n_hi, dtype=f32)
    return (X + F(0.5)) * r - F(0.5)


def unit_normals(n):
    """(n^, has) by the definition's rule; NO NORMAL is (0, 0, 0)"""
    n = np.asarray(n, f32)
    l2 = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
    has = ~(l2 < F(1e-12)) & np.isfinite(l2)
    l = np.sqrt(np.where(has, l2, F(1)))
    return np.where(has[..., None], n / l[..., None], F(0)).astype(f32), has


def falloff(x):
    t = np.fmax(F(0), F(1) - x * F(0.125))
    t = t * t
    t = t * t
    return t * t


def prepare(color, stderr3, albedo, normal, depth, floor):
    """the low planes: I, V, valid, n^, has, z"""
    color = np.asarray(color, f32)
    h, w = color.shape[:2]
    valid = np.isfinite(color).all(-1)
    a = np.fmax(np.asarray(albedo, f32), F(floor)) if albedo is not None else np.ones_like(color)
    with np.errstate(all="ignore"):
        I = color / a
        V = np.zeros_like(color)
        if stderr3 is not None:
            e = np.asarray(stderr3, f32)
            valid &= np.isfinite(e).all(-1)
            s = e / a
            V = s * s
    I = np.where(valid[..., None], I, F(0)).astype(f32)
    V = np.where(valid[..., None], V, F(0)).astype(f32)
    if normal is not None:
        nq, has = unit_normals(normal)
    else:
        nq, has = np.zeros((h, w, 3), f32), np.zeros((h, w), bool)
    z = np.full((h, w), np.inf, f32)
    if depth is not None:
        d = np.asarray(depth, f32).reshape(h, w)
        z = np.where(np.isfinite(d), d, F(np.inf)).astype(f32)
    return I, V, valid, nq, has, z


def slopes(depth_hi):
    """the depth slope in high pixels: minmod of the two one-sided differences, else the one there is, else 0; 0 where the depth is not
    finite"""
    z = np.asarray(depth_hi, f32)
    H, W = z.shape
    inf = F(np.inf)
    zl = np.full_like(z, inf); zl[:, 1:] = z[:, :-1]
    zr = np.full_like(z, inf); zr[:, :-1] = z[:, 1:]
    zd = np.full_like(z, inf); zd[1:] = z[:-1]
    zu = np.full_like(z, inf); zu[:-1] = z[1:]
    fin = np.isfinite(z)
    l, r, d, u = np.isfinite(zl), np.isfinite(zr), np.isfinite(zd), np.isfinite(zu)
    with np.errstate(all="ignore"):
        def slope(has_l, dl, has_r, dr):
            mm = np.where(dl * dr > F(0), np.where(dl > F(0), np.fmin(dl, dr), np.fmax(dl, dr)), F(0))
            return np.where(has_l & has_r, mm, np.where(has_r, dr, np.where(has_l, dl, F(0))))
        gx = slope(l, z - zl, r, zr - z)
        gy = slope(d, z - zd, u, zu - z)
    return np.where(fin, gx, F(0)).astype(f32), np.where(fin, gy, F(0)).astype(f32)


def apply(color, W, H, stderr3=None, albedo=None, normal=None, depth=None, albedo_hi=None, normal_hi=None, depth_hi=None,
          sigma_z=1.0, normal_squarings=7, albedo_floor=1e-3, want_stderr=True):
    """(rgb (H, W, 3), stderr3 (H, W, 3) or None, fallback_pixels, empty_pixels) from an (h, w, 3) low frame, y up"""
    color = np.asarray(color, f32)
    h, w = color.shape[:2]
    assert 2 <= w <= W and 2 <= h <= H
    assert (albedo is None) == (albedo_hi is None)
    assert stderr3 is not None or not want_stderr
    floor, sigma = F(albedo_floor), F(sigma_z)
    I, V, valid, nq, q_has_all, zq_all = prepare(color, stderr3, albedo, normal, depth, floor)
    use_n = normal is not None and normal_hi is not None
    use_z = depth is not None and depth_hi is not None
    rx, sx = ratios(w, W)
    ry, sy = ratios(h, H)
    px, py = centres(W, rx), centres(H, ry)
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    if use_n:
        nP, p_has = unit_normals(np.asarray(normal_hi, f32).reshape(H, W, 3))
    if use_z:
        dh = np.asarray(depth_hi, f32).reshape(H, W)
        zP = np.where(np.isfinite(dh), dh, F(np.inf)).astype(f32)
        gx, gy = slopes(dh)
        p_far = zP == F(np.inf)
    Wg, Jg, Ug = np.zeros((H, W), f32), np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32)
    Wf, Jf, Uf = np.zeros((H, W), f32), np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32)
    with np.errstate(all="ignore"):
        for j in range(4):
            ty = y0 - 1 + j
            in_y = (ty >= 0) & (ty < h)
            tyc = np.clip(ty, 0, h - 1)
            ky = np.fmax(F(0), F(1) - np.abs(py - ty.astype(f32)) * F(0.5))
            for i in range(4):
                tx = x0 - 1 + i
                in_x = (tx >= 0) & (tx < w)
                txc = np.clip(tx, 0, w - 1)
                kx = np.fmax(F(0), F(1) - np.abs(px - tx.astype(f32)) * F(0.5))
                m = in_y[:, None] & in_x[None, :] & valid[tyc][:, txc]
                Iq, Vq = I[tyc][:, txc], V[tyc][:, txc]
                k = kx[None, :] * ky[:, None]
                Wf = np.where(m, Wf + k, Wf)
                Jf = np.where(m[..., None], Jf + k[..., None] * Iq, Jf)
                Uf = np.where(m[..., None], Uf + (k * k)[..., None] * Vq, Uf)
                wn = np.ones((H, W), f32)
                if use_n:
                    n_q, q_has = nq[tyc][:, txc], q_has_all[tyc][:, txc]
                    dot = np.fmax(F(0), (nP[..., 0] * n_q[..., 0] + nP[..., 1] * n_q[..., 1]) + nP[..., 2] * n_q[..., 2])
                    for _ in range(normal_squarings):
                        dot = dot * dot
                    wn = np.where(p_has != q_has, F(0), np.where(p_has, dot, F(1))).astype(f32)
                xz = np.zeros((H, W), f32)
                mg = m
                if use_z:
                    zq = zq_all[tyc][:, txc]
                    q_far = zq == F(np.inf)
                    mg = m & (p_far == q_far)
                    ux = ((tx.astype(f32) - px) * sx)[None, :]
                    uy = ((ty.astype(f32) - py) * sy)[:, None]
                    x = np.abs(zP - zq) / (sigma * (np.abs(gx * ux + gy * uy) + F(0.001) * zP))
                    xz = np.where(p_far, F(0), x).astype(f32)
                wt = (k * wn) * falloff(xz)
                Wg = np.where(mg, Wg + wt, Wg)
                Jg = np.where(mg[..., None], Jg + wt[..., None] * Iq, Jg)
                Ug = np.where(mg[..., None], Ug + (wt * wt)[..., None] * Vq, Ug)
        fb = Wg < F(1e-4)
        Wt = np.where(fb, Wf, Wg)
        J = np.where(fb[..., None], Jf, Jg)
        U = np.where(fb[..., None], Uf, Ug)
        empty = Wt < F(1e-4)
        A = np.fmax(np.asarray(albedo_hi, f32).reshape(H, W, 3), floor) if albedo_hi is not None else np.ones((H, W, 3), f32)
        out = np.where(empty[..., None], F(0), (J / Wt[..., None]) * A).astype(f32)
        se = np.where(empty[..., None], F(0), (np.sqrt(U) / Wt[..., None]) * A).astype(f32) if want_stderr else None
    assert out.dtype == f32 and Wg.dtype == f32 and Jg.dtype == f32 and Ug.dtype == f32
    return out, se, int(fb.sum()), int(empty.sum())
