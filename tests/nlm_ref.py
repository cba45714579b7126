"""numpy restatement of the non-local-means filter, written from include/vecchio_amd.h's text ("non-local means") alone: whole-image
shifts in f32.  A patch sum is built from shifted images — the pair plane of an offset shifted along x and added (the row sums), the
result shifted along y and added — not from the kernel's loops.  TESTS ONLY."""
import numpy as np

f32 = np.float32


def shift(img, ox, oy, fill):
    """S[y, x] = img[y + oy, x + ox], `fill` where that is outside the image"""
    H, W = img.shape[:2]
    out = np.full_like(img, fill)
    ys, ye = max(0, -oy), min(H, H - oy)
    xs, xe = max(0, -ox), min(W, W - ox)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = img[ys + oy:ye + oy, xs + ox:xe + ox]
    return out


def falloff(x):
    t = np.fmax(f32(0), f32(1) - x * f32(0.125))
    t = t * t
    t = t * t
    return t * t


def prepare(color, stderr3, albedo, albedo_floor):
    """(I, V, Vf, a, valid): (H, W, 3) float32 each, valid (H, W) bool"""
    color, stderr3 = np.asarray(color, f32), np.asarray(stderr3, f32)
    with np.errstate(all="ignore"):
        a = np.ones_like(color) if albedo is None else np.fmax(np.asarray(albedo, f32), f32(albedo_floor))
        I = color / a
        s = stderr3 / a
        V = s * s
        valid = np.isfinite(color).all(axis=2) & np.isfinite(stderr3).all(axis=2)
        acc, ws = np.zeros_like(V), np.zeros(V.shape[:2], f32)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                kw = f32((2 if dx == 0 else 1) * (2 if dy == 0 else 1))
                vq = shift(valid, dx, dy, False)
                acc = np.where(vq[..., None], acc + kw * shift(V, dx, dy, f32(0)), acc)
                ws = np.where(vq, ws + kw, ws)
        Vf = acc / ws[..., None]
    return I, V, Vf, a, valid


def filter(color, stderr3, albedo=None, R=7, F=3, k=0.45, alpha=1.0, albedo_floor=1e-3):
    """(out, stderr3_out), (H, W, 3) float32, y up"""
    color, stderr3 = np.asarray(color, f32), np.asarray(stderr3, f32)
    I, V, Vf, a, valid = prepare(color, stderr3, albedo, albedo_floor)
    alpha, kk = f32(alpha), f32(k) * f32(k)
    H, Wd = valid.shape
    W = np.zeros((H, Wd), f32)
    J, U = np.zeros((H, Wd, 3), f32), np.zeros((H, Wd, 3), f32)
    with np.errstate(all="ignore"):
        for oy in range(-R, R + 1):
            for ox in range(-R, R + 1):
                vq = shift(valid, ox, oy, False)
                take = valid & vq
                Iq, Vq = shift(I, ox, oy, f32(0)), shift(V, ox, oy, f32(0))
                if ox == 0 and oy == 0:
                    w = np.ones((H, Wd), f32)
                else:
                    Vfq = shift(Vf, ox, oy, f32(0))
                    d = I - Iq
                    num = d * d - alpha * (Vf + np.fmin(Vf, Vfq))
                    den = f32(1e-10) + kk * (Vf + Vfq)
                    t = num / den
                    E = np.where(take, (t[..., 0] + t[..., 1]) + t[..., 2], f32(0)).astype(f32)
                    Cn = take.astype(np.int64)
                    rows, rows_n = np.zeros((H, Wd), f32), np.zeros((H, Wd), np.int64)
                    for i in range(-F, F + 1):
                        rows = rows + shift(E, i, 0, f32(0))
                        rows_n = rows_n + shift(Cn, i, 0, 0)
                    S, n = np.zeros((H, Wd), f32), np.zeros((H, Wd), np.int64)
                    for j in range(-F, F + 1):
                        S = S + shift(rows, 0, j, f32(0))
                        n = n + shift(rows_n, 0, j, 0)
                    D = S / (3 * np.maximum(n, 1)).astype(f32)
                    w = np.where(np.isnan(D), f32(0), falloff(np.fmax(f32(0), D))).astype(f32)
                W = np.where(take, W + w, W)
                J = np.where(take[..., None], J + w[..., None] * Iq, J)
                U = np.where(take[..., None], U + (w * w)[..., None] * Vq, U)
        out = (J / W[..., None]) * a
        se = (np.sqrt(U) / W[..., None]) * a
    out = np.where(valid[..., None], out, color).astype(f32)
    se = np.where(valid[..., None], se, stderr3).astype(f32)
    return out, se


def same_bits(a, b):
    """bit for bit, a NaN's payload aside"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | nan).all())


def synthetic(W, H, seed):
    """random colours over a smooth ramp with a heteroscedastic standard error, and an albedo: (color, stderr3, albedo)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([0.2 + 0.8 * x / max(W - 1, 1), 0.5 + 0.4 * np.sin(0.7 * y), 0.3 + 0.02 * (x + y)], axis=2)
    albedo = (0.1 + 0.9 * rng.random((H, W, 3))).astype(f32)
    sigma = (0.02 + 0.3 * rng.random((H, W, 3))) * base
    color = (base + sigma * rng.standard_normal((H, W, 3))).astype(f32) * albedo
    return color.astype(f32), (sigma * albedo).astype(f32), albedo


def special_cases(W, H, seed):
    """name -> (color, stderr3, albedo) over synthetic(): non-finite pixels singly and as a block larger than a patch, zero stderr next
    to noise (the 1e-10f path; with far-apart colours D = +inf), albedo 0 (the floor), values whose d * d overflows next to variances
    that overflow (inf - inf: the NaN rule)"""
    out = {}
    c, s, a = synthetic(W, H, seed)
    out["plain"] = (c, s, a)
    c1, s1 = c.copy(), s.copy()
    c1[H // 2, W // 2, 1] = np.nan
    c1[0, 0, 0] = np.inf
    s1[H - 1, W - 1, 2] = -np.inf
    s1[H // 3, (2 * W) // 3, 0] = np.nan
    out["nonfinite_single"] = (c1, s1, a)
    c2, s2 = c.copy(), s.copy()
    c2[1:min(H, 10), 2:min(W, 11)] = np.nan                 # up to 9 x 9: larger than a 7 x 7 patch
    s2[:, W - 1:] = np.inf
    out["nonfinite_block"] = (c2, s2, a)
    c3, s3 = c.copy(), s.copy()
    s3[:, : (W + 1) // 2] = 0.0
    c3[:, : (W + 3) // 4] = f32(3e15) * (1 + np.arange(H, dtype=f32))[:, None, None]      # zero variance, far apart: num / 1e-10 = +inf
    out["zero_stderr"] = (c3, s3, a)
    a4 = a.copy()
    a4[::2, ::3] = 0.0
    a4[H // 2:, 0] = -1.0
    out["albedo_zero"] = (c, s, a4)
    c5, s5 = c.copy(), s.copy()
    c5[:, ::2] = f32(1e30)
    c5[:, 1::4] = f32(-1e30)
    s5[: (H + 1) // 2] = f32(1e25)
    out["overflow"] = (c5, s5, None)
    return out


def rel_mse(x, t):
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    return float(np.mean((x - t) ** 2 / (t ** 2 + 0.01)))
