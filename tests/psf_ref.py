"""numpy restatement of the point-spread stage, written from include/vecchio_amd.h's text ("point-spread function") alone: every
butterfly of a stage of every line at once, in f32, one rounding per numpy operation as the device has one per instruction.  The tables
and the kernel's normalisation are f64.  TESTS ONLY."""
import math

import numpy as np

f32 = np.float32


def pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def padded(W, H, K):
    return pow2(W + K - 1), pow2(H + K - 1)


def twiddles(N):
    """(N / 2, 2) float32 (re, im): the header's rule in f64 — + - * / and sqrt, all correctly rounded, as Python floats and numpy
    float64 elementwise operations are"""
    m = N.bit_length() - 1
    c, s = {1: 0.0}, {1: 1.0}
    for q in range(1, 15):
        c[q + 1] = math.sqrt((1.0 + c[q]) / 2.0)
        s[q + 1] = s[q] / (2.0 * c[q + 1])
    k = np.arange(N // 2)
    zr, zi = np.ones(N // 2, np.float64), np.zeros(N // 2, np.float64)
    for t in range(0, m - 1):
        q = m - 1 - t
        on = (k >> t) & 1 == 1
        nr = zr * c[q] - zi * s[q]
        ni = zr * s[q] + zi * c[q]
        zr, zi = np.where(on, nr, zr), np.where(on, ni, zi)
    return np.stack([zr.astype(f32), (0.0 - zi).astype(f32)], axis=1)


def rev(N):
    m = N.bit_length() - 1
    i = np.arange(N)
    r = np.zeros(N, np.int64)
    for b in range(m):
        r |= ((i >> b) & 1) << (m - 1 - b)
    return r


def fft_last_axis(re, im, inverse=False):
    """the 1-D transform of every line along the last axis; re, im float32 arrays of the same shape"""
    N = re.shape[-1]
    m = N.bit_length() - 1
    T = twiddles(N) if N >= 2 else np.zeros((0, 2), f32)
    r = rev(N)
    # a[rev(i)] = input[i]; rev is an involution
    re, im = np.ascontiguousarray(re[..., r], f32), np.ascontiguousarray(im[..., r], f32)
    lead = re.shape[:-1]
    with np.errstate(all="ignore"):
        for s in range(1, m + 1):
            half = 1 << (s - 1)
            w = T[(np.arange(half) * (N >> s))]
            wr, wi = w[:, 0], (-w[:, 1] if inverse else w[:, 1])
            re = re.reshape(lead + (N >> s, 2, half))
            im = im.reshape(lead + (N >> s, 2, half))
            ur, ui, vr, vi = re[..., 0, :], im[..., 0, :], re[..., 1, :], im[..., 1, :]
            tr = vr * wr - vi * wi
            ti = vr * wi + vi * wr
            re = np.stack([ur + tr, ur - tr], axis=-2).reshape(lead + (N,))
            im = np.stack([ui + ti, ui - ti], axis=-2).reshape(lead + (N,))
    return re.astype(f32), im.astype(f32)


def fft2(re, im, inverse=False, scale=True):
    """(Py, Px) planes: rows along x, then columns along y; the inverse ends with one multiplication by 1 / (Px Py) if `scale`"""
    Py, Px = re.shape
    re, im = fft_last_axis(np.asarray(re, f32), np.asarray(im, f32), inverse)
    re, im = fft_last_axis(re.T, im.T, inverse)
    re, im = np.ascontiguousarray(re.T), np.ascontiguousarray(im.T)
    if inverse and scale:
        sc = f32(1.0) / (f32(Px) * f32(Py))
        re, im = re * sc, im * sc
    return re, im


def bright(I, threshold):
    """B of an (H, W, 3) frame: vk_glare's"""
    T = f32
    I = np.asarray(I, T)
    with np.errstate(all="ignore"):
        s = np.where(I > 0, np.where(I < T(1048576.0), I, T(1048576.0)), T(0)).astype(T)
        if threshold != 0:
            Y = (T(0.2126) * s[..., 0] + T(0.7152) * s[..., 1]) + T(0.0722) * s[..., 2]
            f = np.fmax(T(0), Y - T(threshold)) / np.fmax(Y, T(1e-20))
            s = s * f[..., None]
    fin = np.isfinite(I).all(axis=2)
    return np.where(fin[..., None], s, T(0)).astype(T)


def normalise(kernel):
    """the (K, K, 3) kernel as a load keeps it, or ValueError"""
    k = np.asarray(kernel, f32)
    if not np.isfinite(k).all():
        raise ValueError("kernel component not finite")
    if (k < 0).any():
        raise ValueError("kernel component negative")
    out = np.zeros_like(k)
    for c in range(3):
        S = 0.0
        for v in k[..., c].ravel().astype(np.float64):       # ascending index order
            S += float(v)
        if not S > 0.0:
            raise ValueError("kernel channel sums to nothing")
        out[..., c] = (k[..., c].astype(np.float64) / S).astype(f32)
    return out


def placed(kc, Px, Py):
    """one channel of the normalised kernel, (K, K) indexed [ky, kx], in a (Py, Px) plane with its centre at (0, 0), wrapped"""
    K = kc.shape[0]
    r = (K - 1) // 2
    g = np.zeros((Py, Px), f32)
    idx = np.arange(K) - r
    g[np.ix_(idx % Py, idx % Px)] = kc
    return g


def spread(I, kernel, threshold=0.0):
    """(C, B) of an (H, W, 3) frame: the convolution at the frame's pixels and the bright part"""
    I = np.asarray(I, f32)
    H, W = I.shape[:2]
    k = normalise(kernel)
    K = k.shape[0]
    Px, Py = padded(W, H, K)
    B = bright(I, threshold)
    C = np.zeros_like(B)
    sc = f32(1.0) / (f32(Px) * f32(Py))
    with np.errstate(all="ignore"):
        for c in range(3):
            b = np.zeros((Py, Px), f32)
            b[:H, :W] = B[..., c]
            Fr, Fi = fft2(b, np.zeros_like(b))
            g = placed(k[..., c], Px, Py)
            Gr, Gi = fft2(g, np.zeros_like(g))
            Pr = Fr * Gr - Fi * Gi
            Pi = Fr * Gi + Fi * Gr
            Cr, _ = fft2(Pr, Pi, inverse=True, scale=False)
            C[..., c] = Cr[:H, :W] * sc
    return C, B


def apply(I, kernel, strength=0.15, threshold=0.0):
    """out of an (H, W, 3) frame, y up"""
    I = np.asarray(I, f32)
    C, B = spread(I, kernel, threshold)
    with np.errstate(all="ignore"):
        out = (I + f32(strength) * (C - B)).astype(f32)
    return np.where(np.isfinite(I), out, I)


def same_floats(a, b):
    """bit for bit as floats: -0 equal to +0, a NaN's payload aside"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(((a == b) | nan).all())
