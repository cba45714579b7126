"""numpy restatement of the glare stage, written from include/vecchio_amd.h's text ("glare") alone: whole-image gathers along one axis at a
time, in f32; dtype=np.float64 gives the same operator in f64 (the weights are then p_l / S unrounded, the constants the f64 values of
the same decimals).  TESTS ONLY."""
import numpy as np

f32 = np.float32


def weights(levels, falloff, dtype=f32):
    """c_0 .. c_{L-1}: f64 basic arithmetic, falloff as the f32 the library receives"""
    fo = float(f32(falloff))
    p = [1.0]
    for _ in range(1, levels):
        p.append(p[-1] * fo)
    S = 0.0
    for v in p:
        S += v
    return [dtype(v / S) for v in p]


def sizes(W, H, levels):
    out = [(W, H)]
    for _ in range(1, levels):
        w, h = out[-1]
        out.append(((w + 1) // 2, (h + 1) // 2))
    return out


def bright(I, threshold, dtype=f32):
    """B of an (H, W, 3) frame"""
    T = dtype
    I = np.asarray(I, T)
    with np.errstate(all="ignore"):
        s = np.where(I > 0, np.where(I < T(1048576.0), I, T(1048576.0)), T(0)).astype(T)
        if threshold != 0:
            Y = (T(0.2126) * s[..., 0] + T(0.7152) * s[..., 1]) + T(0.0722) * s[..., 2]
            f = np.fmax(T(0), Y - T(threshold)) / np.fmax(Y, T(1e-20))
            s = s * f[..., None]
    fin = np.isfinite(I).all(axis=2)
    return np.where(fin[..., None], s, T(0)).astype(T)


def _down_axis(a, axis):
    T = a.dtype.type
    n = a.shape[axis]
    j = np.arange((n + 1) // 2)
    tap = lambda o: np.take(a, np.clip(2 * j + o, 0, n - 1), axis=axis)
    return ((tap(-1) + T(3) * tap(0)) + (T(3) * tap(1) + tap(2))) * T(0.125)


def down(a):
    """(h, w, 3) -> (ceil(h / 2), ceil(w / 2), 3): x first, then y"""
    return _down_axis(_down_axis(a, 1), 0)


def _up_axis(a, axis, n_out):
    T = a.dtype.type
    n = a.shape[axis]
    x = np.arange(n_out)
    j = x >> 1
    nb = np.clip(np.where(x & 1, j + 1, j - 1), 0, n - 1)
    return (T(3) * np.take(a, j, axis=axis) + np.take(a, nb, axis=axis)) * T(0.25)


def up(a, w, h):
    """(., ., 3) -> (h, w, 3): x first, then y"""
    return _up_axis(_up_axis(a, 1, w), 0, h)


def spread(I, levels=6, falloff=1.0, threshold=0.0, dtype=f32):
    """(A_0, B): the weighted sum of the pyramid at level 0 and the bright part"""
    c = weights(levels, falloff, dtype)
    with np.errstate(all="ignore"):
        B = [bright(I, threshold, dtype)]
        for _ in range(1, levels):
            B.append(down(B[-1]))
        A = c[levels - 1] * B[levels - 1]
        for l in range(levels - 2, -1, -1):
            h, w = B[l].shape[:2]
            A = c[l] * B[l] + up(A, w, h)
    return A, B[0]


def apply(I, levels=6, strength=0.15, falloff=1.0, threshold=0.0, dtype=f32):
    """out of an (H, W, 3) frame, y up"""
    T = dtype
    I = np.asarray(I, T)
    A0, B = spread(I, levels, falloff, threshold, dtype)
    with np.errstate(all="ignore"):
        return (I + T(strength) * (A0 - B)).astype(T)


def same_bits(a, b):
    """bit for bit, a NaN's payload aside"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | nan).all())


def hdr_frame(W, H, seed, special=True):
    """a random HDR frame: log-uniform radiances over twelve octaves with a few lamps; with `special`, NaN, +-inf, -0, negatives and
    values above 2^20 sown in"""
    rng = np.random.default_rng(seed)
    I = np.exp2(rng.uniform(-8, 4, (H, W, 3))).astype(f32)
    n = W * H
    flat = I.reshape(n, 3)
    for k in rng.integers(0, n, max(1, n // 50)):
        flat[k] = f32(rng.uniform(50, 5000))
    if special:
        vals = [np.nan, np.inf, -np.inf, -0.0, -3.5, 3e6, 1048576.0, 0.0, 1e-30, -np.nan]
        for i, v in enumerate(vals):
            flat[rng.integers(0, n), i % 3] = f32(v)
        flat[rng.integers(0, n)] = f32(2e7)
    return I


def lamp_frame(W, H, seed, levels):
    """a frame whose outer 3 * 2^(levels - 1) pixels are black, values well inside (2^-10, 2^10): nothing reaches the border's clamp"""
    rng = np.random.default_rng(seed)
    m = 3 * 2 ** (levels - 1)
    assert W > 2 * m and H > 2 * m
    I = np.zeros((H, W, 3), f32)
    I[m:H - m, m:W - m] = np.exp2(rng.uniform(-6, 8, (H - 2 * m, W - 2 * m, 3))).astype(f32)
    return I
