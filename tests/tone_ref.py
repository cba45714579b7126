"""vk_tone_meter, vk_tone_solve and vk_tone_encode restated from the definition in include/vecchio_amd.h ("display transform"): the
histogram and the encode in numpy — every f32 operation one numpy operation on float32 arrays —, the exposure in plain Python floats and
math.ldexp, the tables and the closed form of contract 6 in float64.  What tests/test_tone_emu.py and tests/test_gpu_tone.py share."""
import math

import numpy as np

from vecchio_amd import ffi

f32 = np.float32
u64 = np.uint64
CLAMP, REINHARD, HABLE, ACES = ffi.VK_TONE_CLAMP, ffi.VK_TONE_REINHARD, ffi.VK_TONE_HABLE, ffi.VK_TONE_ACES
CURVES = (CLAMP, REINHARD, HABLE, ACES)
REFERENCE, SRGB, GAMMA22 = ffi.VK_TONE_TRANSFER_REFERENCE, ffi.VK_TONE_TRANSFER_SRGB, ffi.VK_TONE_TRANSFER_GAMMA22
TRANSFERS = (REFERENCE, SRGB, GAMMA22)
BINS = 640
COUNTERS = ("binned", "below", "above", "nonfinite")
Y_MIN, Y_MAX = f32(2.0 ** -20), f32(2.0 ** 20)
BIN_BASE = int(np.array(Y_MIN).view(np.uint32)) >> 19


def luminance(r, g, b):
    return ((f32(0.2126) * r + f32(0.7152) * g).astype(f32) + f32(0.0722) * b).astype(f32)


# ---------------------------------------------------------------- histogram
def histogram(rgb):
    """(bins (640,) uint32, counters (4,) uint64: binned, below, above, nonfinite) of rgb (..., 3) float32"""
    rgb = np.ascontiguousarray(rgb, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        finite = np.isfinite(rgb).all(axis=1)
        Y = luminance(rgb[:, 0], rgb[:, 1], rgb[:, 2])
        below = finite & ~(Y >= Y_MIN)
        above = finite & ~below & (Y >= Y_MAX)
        binned = finite & ~below & ~above
    idx = (Y[binned].view(np.uint32) >> 19).astype(np.int64) - BIN_BASE
    assert ((idx >= 0) & (idx < BINS)).all()
    bins = np.bincount(idx, minlength=BINS).astype(np.uint32)
    return bins, np.array([binned.sum(), below.sum(), above.sum(), (~finite).sum()], u64)


# ---------------------------------------------------------------- exposure
def pexp2(x):
    e = math.floor(x)
    return math.ldexp(1.0 + (x - e), int(e))


def solve(bins, mp, prev=None):
    """vk_tone_solve in Python floats: dict(log2_target, log2_used, exposure (np.float32), flags, binned)"""
    key, low, high, blend = float(f32(mp.key)), float(f32(mp.low_fraction)), float(f32(mp.high_fraction)), float(f32(mp.blend))
    mn, mx = float(f32(mp.min_log2)), float(f32(mp.max_log2))
    N = int(np.asarray(bins, np.uint64).sum())
    lo, hi = low * float(N), (1.0 - high) * float(N)
    S = W = c = 0.0
    for b in range(BINS):
        nxt = c + float(int(bins[b]))
        w = max(0.0, min(nxt, hi) - max(c, lo))
        l = -20.0 + (b + 0.5) / 16.0
        S += w * l
        W += w
        c = nxt
    clamp = lambda u: mn if u < mn else (mx if u > mx else u)
    if N == 0 or not W > 0.0:
        if prev is None:
            return dict(log2_target=0.0, log2_used=0.0, exposure=f32(1.0), flags=ffi.VK_TONE_METER_EMPTY, binned=N)
        u = clamp(prev)
        return dict(log2_target=prev, log2_used=u, exposure=f32(key * pexp2(-u)), flags=ffi.VK_TONE_METER_EMPTY, binned=N)
    target = S / W
    u = clamp(prev + blend * (target - prev) if prev is not None else target)
    return dict(log2_target=target, log2_used=u, exposure=f32(key * pexp2(-u)), flags=0, binned=N)


def info_dict(info):
    return dict(log2_target=float(info.log2_target), log2_used=float(info.log2_used), exposure=f32(info.exposure), flags=int(info.flags),
                binned=int(info.binned))


def same_info(a, b):
    """bit for bit: the doubles by their bytes (so that -0.0 and NaN cannot hide), the float, the integers"""
    pack = lambda d: (np.float64(d["log2_target"]).tobytes(), np.float64(d["log2_used"]).tobytes(), f32(d["exposure"]).tobytes(),
                      d["flags"], d["binned"])
    return pack(a) == pack(b)


# ---------------------------------------------------------------- tables
def inverse64(transfer, c):
    c = np.asarray(c, np.float64)
    if transfer == SRGB:
        return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    return c ** 2.2


def table64(transfer):
    """the test's own float64 values inv(j / 510), j = 1 .. 510"""
    return inverse64(transfer, np.arange(1, 511, dtype=np.float64) / 510.0)


def oetf64(transfer, y):
    y = np.clip(np.asarray(y, np.float64), 0.0, 1.0)
    if transfer == SRGB:
        return np.where(y <= 0.0031308, 12.92 * y, 1.055 * y ** (1.0 / 2.4) - 0.055)
    return y ** (1.0 / 2.2)


# ---------------------------------------------------------------- the dither's generator (vk_math.h rng_for_stream, next_u32, gen_f32)
def mix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
        return z ^ (z >> u64(31))


def dither_draws(seed, pixels):
    """(n, 3) float32: the first three gen_f32 of rng_for_stream(seed, pixel) for every pixel"""
    pixels = np.asarray(pixels, u64)
    with np.errstate(over="ignore"):
        h = mix64(np.array([seed], u64) + u64(0x9E3779B97F4A7C15))
        key = mix64(h ^ mix64(pixels + u64(0xD1B54A32D192ED03)))
        out = np.zeros((len(pixels), 3), f32)
        for c in range(3):
            z = key + u64(c + 1) * u64(0x9E3779B97F4A7C15)
            u = (mix64(z) >> u64(32)).astype(np.uint32)
            out[:, c] = (u >> np.uint32(8)).astype(f32) * f32(1.0 / 16777216.0)
    return out


# ---------------------------------------------------------------- encode
def hable(v):
    A, B, C, D, E_, F = f32(0.15), f32(0.5), f32(0.1), f32(0.2), f32(0.02), f32(0.3)
    v = np.asarray(v, f32)
    num = ((v * ((A * v).astype(f32) + (C * B)).astype(f32)).astype(f32) + D * E_).astype(f32)
    den = ((v * ((A * v).astype(f32) + B).astype(f32)).astype(f32) + D * F).astype(f32)
    return ((num / den).astype(f32) - E_ / F).astype(f32)


def curve_param(curve, white):
    """what the host hands the kernel: REINHARD white * white, HABLE h(white), else 0"""
    white = f32(white)
    with np.errstate(all="ignore"):
        if curve == REINHARD:
            return f32(white * white)
        if curve == HABLE:
            return f32(hable(white))
    return f32(0.0)


def sanitise(x):
    big = f32(1048576.0)
    return np.where(x > 0, np.where(x < big, x, big), f32(0.0)).astype(f32)


def curve(x, which, p):
    """x (n, 3) float32 = rgb * E -> y (n, 3) float32"""
    if which == CLAMP:
        return x
    s = sanitise(x)
    one = f32(1.0)
    if which == REINHARD:
        Ys = luminance(s[:, 0], s[:, 1], s[:, 2])
        k = ((one + (Ys / p).astype(f32)).astype(f32) / (one + Ys).astype(f32)).astype(f32)
        return (s * k[:, None]).astype(f32)
    if which == HABLE:
        return (hable((f32(2.0) * s).astype(f32)) / p).astype(f32)
    num = (s * ((f32(2.51) * s).astype(f32) + f32(0.03)).astype(f32)).astype(f32)
    den = ((s * ((f32(2.43) * s).astype(f32) + f32(0.59)).astype(f32)).astype(f32) + f32(0.14)).astype(f32)
    return (num / den).astype(f32)


def code_reference(y):
    v = np.sqrt(y).astype(f32)
    cl = np.where(v < 0, f32(0.0), np.where(v > f32(0.999), f32(0.999), v)).astype(f32)
    m = (f32(256.0) * cl).astype(f32)
    return np.where(m > 0, np.where(m > 0, m, 0).astype(np.int64), 0).astype(np.uint32) & np.uint32(255)


def count_at_least(thresholds, y):
    """#{k : y >= thresholds[k]} for ascending thresholds; a NaN counts none"""
    n = np.searchsorted(thresholds, y, side="right")
    return np.where(np.isnan(y), 0, n).astype(np.uint32)


def code_table(H, y):
    return count_at_least(H[0::2][:255], y)                       # H[2k - 1] = H[0], H[2], .. in 0-based terms


def code_dither(H, y, u):
    base = count_at_least(H[1::2][:255], y)                       # H[2k]
    at = np.minimum(base, 254).astype(np.int64)
    lo = np.where(at > 0, H[np.maximum(2 * at - 1, 0)], f32(0.0)).astype(f32)
    hi = H[2 * at + 1]
    fr = ((y - lo).astype(f32) / (hi - lo).astype(f32)).astype(f32)
    return np.where(base < 255, base + (u < fr), 255).astype(np.uint32)


def encode(rgb, which, table, dither, E, p, seed=0):
    """vk_tone_encode in numpy: rgb (H, W, 3) float32, y up; table: the library's 510 thresholds (vk_debug_tone_table) or None for the
    reference transfer; E, p: what the host computes (params.exposure * metered, curve_param) -> (H, W, 3) uint8, row 0 the top"""
    rgb = np.ascontiguousarray(rgb, f32)
    Hh, W = rgb.shape[:2]
    with np.errstate(all="ignore"):
        x = (rgb.reshape(-1, 3) * f32(E)).astype(f32)
        y = curve(x, which, f32(p))
        if table is None:
            code = code_reference(y)
        else:
            T = np.ascontiguousarray(table, f32)
            if not dither:
                code = code_table(T, y)
            else:
                code = code_dither(T, y, dither_draws(seed, np.arange(Hh * W)))
    return code.astype(np.uint8).reshape(Hh, W, 3)[::-1].copy()


def closed_form(rgb, which, transfer, E, white):
    """contract 6's reference in float64: round(255 * OETF(curve(E * x))), rgb (n, 3) -> (n, 3) int64, in the input's order"""
    x = np.asarray(rgb, np.float64).reshape(-1, 3) * float(f32(E))
    w = float(f32(white))
    if which == CLAMP:
        y = x
    else:
        s = np.where(x > 0, np.minimum(x, 1048576.0), 0.0)
        if which == REINHARD:
            Ys = 0.2126 * s[:, 0] + 0.7152 * s[:, 1] + 0.0722 * s[:, 2]
            y = s * ((1.0 + Ys / (w * w)) / (1.0 + Ys))[:, None]
        elif which == HABLE:
            A, B, C, D, E_, F = 0.15, 0.5, 0.1, 0.2, 0.02, 0.3
            h = lambda v: (v * (A * v + C * B) + D * E_) / (v * (A * v + B) + D * F) - E_ / F
            y = h(2.0 * s) / h(w)
        else:
            y = (s * (2.51 * s + 0.03)) / (s * (2.43 * s + 0.59) + 0.14)
    return np.floor(255.0 * oetf64(transfer, y) + 0.5).astype(np.int64)


# ---------------------------------------------------------------- frames
def specials(table=None):
    """(n, 3) float32 pixels that hold everything the kernels branch on: NaN, +-inf, -0, negatives, denormals; 2^-20 and 2^20 and their
    neighbours by one ulp; every bin edge of three octaves +- one ulp (as grey, whose luminance is the value up to rounding, and as a pure
    green of that luminance); the table's thresholds +- one ulp"""
    nxt = lambda v, d: np.nextafter(f32(v), f32(d))
    vals = [np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, -1e-30, 1e-40, -1e-40, 1.4e-45, 1.0, 0.999, 0.5, 255.0, 3e38, -3e38]
    for v in (2.0 ** -20, 2.0 ** 20, 1.0, 0.998001, 0.999 ** 2):
        vals += [nxt(v, 0), v, nxt(v, np.inf)]
    for octave in (-20, -1, 19):
        for k in range(17):
            e = f32(2.0 ** octave * (1.0 + k / 16.0))
            vals += [nxt(e, 0), e, nxt(e, np.inf)]
    if table is not None:
        for t in np.asarray(table, f32):
            vals += [nxt(t, 0), t, nxt(t, np.inf)]
    vals = np.array(vals, f32)
    grey = np.repeat(vals[:, None], 3, axis=1)
    with np.errstate(all="ignore"):
        green = np.zeros((len(vals), 3), f32)
        green[:, 1] = (vals / f32(0.7152)).astype(f32)
    mixed = grey.copy()
    mixed[:, 0] = np.roll(vals, 1)
    mixed[:, 2] = np.roll(vals, 5)
    return np.concatenate([grey, green, mixed]).astype(f32)


def frame_of(pixels, width, height):
    """the pixels (n, 3), repeated as often as it takes, as a frame (height, width, 3)"""
    n = width * height
    reps = -(-n // len(pixels))
    return np.ascontiguousarray(np.tile(pixels, (reps, 1))[:n].reshape(height, width, 3), f32)


def noise(width, height, seed, lo=-15.0, hi=15.0):
    """log-uniform noise over hi - lo octaves, each component its own"""
    rng = np.random.default_rng(seed)
    return np.exp2(rng.uniform(lo, hi, (height, width, 3))).astype(f32)
