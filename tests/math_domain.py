"""Inputs and the correctly rounded reference for the whole-domain checks of the shared arithmetic (vecchio_amd/csrc/vk_math.h):
tests/test_math_domain.py holds the host build to the reference, tests/test_gpu_parity.py the device to the host on the same inputs.

correctly_rounded(fn, x[, y]) is the f32 nearest to the true value: float64 numpy rounded to f32, and mpmath at 200 bits wherever
the float64 value lies within 2^-20 f32 ulp of a rounding tie (float64 functions are good to a few 2^-52; the window is 2^8 times
wider than the 2^-28 that would suffice for a 1-ulp float64 libm)."""
import mpmath
import numpy as np

F32_MAX = float(np.finfo(np.float32).max)
OVERFLOW = 2.0 ** 128 - 2.0 ** 103           # f32 rounding boundary to inf
TIE_WINDOW = 2.0 ** -20                      # in f32 ulps
SWEEP_STRIDE = 61                            # prime: every 61st of the 2^32 bit patterns, ~70 M inputs
CHUNK = 1 << 22

UNARY = ("sin", "cos", "log", "asin", "pow5")
OP = {"sin": 0, "cos": 1, "log": 2, "asin": 3, "atan2": 4, "pow5": 5, "sincos.s": 11, "sincos.c": 12, "sincos_small.s": 13,
      "sincos_small.c": 14}

_NP = {"sin": np.sin, "cos": np.cos, "log": np.log, "asin": np.arcsin, "pow5": lambda x: np.power(x, 5.0), "atan2": np.arctan2}
_MP = {"sin": mpmath.sin, "cos": mpmath.cos, "log": mpmath.log, "asin": mpmath.asin, "pow5": lambda x: x ** 5, "atan2": mpmath.atan2}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def floats(u):
    return np.asarray(u, np.uint32).view(np.float32)


def ulp_index(a):
    """a monotone integer image of f32 (-0 and +0 both 0): ulp distances are differences"""
    i = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def same(got, want):
    """bit-equal, or both NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def _mp_value(fn, x, y):
    if fn == "atan2":
        return _MP[fn](mpmath.mpf(float(x)), mpmath.mpf(float(y)))
    return _MP[fn](mpmath.mpf(float(x)))


def _mp_round_f32(v):
    """round an mpmath real to the nearest f32, ties to even"""
    if mpmath.isnan(v):
        return np.float32(np.nan)
    if abs(v) >= OVERFLOW:
        return np.float32(np.inf) if v > 0 else np.float32(-np.inf)
    with np.errstate(over="ignore"):
        c = np.float32(float(v))
    cands = {np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))}
    cands = [k for k in cands if np.isfinite(k)]
    best = min(cands, key=lambda k: (abs(v - mpmath.mpf(float(k))), int(bits(k)) & 1))
    if best == 0 and v < 0:
        best = np.float32(-0.0)
    return np.float32(best)


def correctly_rounded(fn, x, y=None, undecided_out=None):
    """the correctly rounded f32 value of fn at the f32 inputs x (and y for atan2(x, y)).  Where float64 cannot decide (within
    TIE_WINDOW of a tie, or of the overflow boundary), mpmath at 200 bits does; undecided_out (a list) receives their count."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        x64 = x.astype(np.float64)
        if fn == "atan2":
            y = np.asarray(y, np.float32)
            v = _NP[fn](x64, y.astype(np.float64))
        else:
            v = _NP[fn](x64)
        out = v.astype(np.float32)
        o64 = out.astype(np.float64)
        o64 = np.where(np.isinf(out) & np.isfinite(v), np.sign(v) * 2.0 ** 128, o64)     # inf as the boundary's far side
        d = v - o64
        toward = np.where(d > 0, np.inf, -np.inf).astype(np.float32)
        nb = np.nextafter(out, toward).astype(np.float64)
        nb = np.where(np.isinf(nb) & np.isfinite(o64), np.sign(o64) * 2.0 ** 128, nb)
        nb = np.where(np.isinf(out) & np.isfinite(v), np.sign(v) * F32_MAX, nb)
        ulp = np.abs(nb - o64)
        mid = 0.5 * (o64 + nb)
        undecided = np.isfinite(v) & (d != 0) & (np.abs(v - mid) <= TIE_WINDOW * ulp)
    idx = np.nonzero(undecided)[0]
    if idx.size:
        with mpmath.workprec(200):
            for i in idx:
                out[i] = _mp_round_f32(_mp_value(fn, x[i], None if y is None else y[i]))
    if undecided_out is not None:
        undecided_out.append(int(idx.size))
    return out


def sweep_chunks(stride=SWEEP_STRIDE, chunk=CHUNK):
    """every stride-th of the 2^32 bit patterns (both signs, subnormals, inf, NaN), in chunks"""
    n = ((1 << 32) + stride - 1) // stride
    for k0 in range(0, n, chunk):
        k = np.arange(k0, min(n, k0 + chunk), dtype=np.uint64)
        yield floats((k * stride).astype(np.uint32))


def range_chunks(lo, hi, stride=1, chunk=CHUNK):
    """every stride-th f32 with bit pattern in [bits(lo), bits(hi)) for 0 <= lo < hi"""
    b0, b1 = int(bits(np.float32(lo))), int(bits(np.float32(hi)))
    for s in range(b0, b1, chunk * stride):
        yield floats(np.arange(s, min(b1, s + chunk * stride), stride, dtype=np.uint64).astype(np.uint32))


def sampler_angles():
    """every 31st f32 in [0, 2 pi): the angles 2 pi u of the samplers"""
    return range_chunks(0.0, np.float32(2 * np.pi), stride=31)


def asin_near_one():
    """every f32 with 1 - 2^-10 <= |x| <= 1"""
    x = np.concatenate(list(range_chunks(1.0 - 2.0 ** -10, np.nextafter(np.float32(1), np.float32(2)))))
    return np.concatenate([x, -x])


def log_ranges():
    """every f32 in [0.5, 2] and in [2^-24, 2^-20), every 97th in (0, 2^-24)"""
    yield from range_chunks(0.5, np.nextafter(np.float32(2), np.float32(3)))
    yield from range_chunks(2.0 ** -24, 2.0 ** -20)
    yield from range_chunks(1e-45, 2.0 ** -24, stride=97)


def specials():
    """signed zeros, subnormals, the normal boundary, ones, the largest finite values, inf, NaN, and the neighbours of the
    reduction's switch at 2^22 and of the old 1e9 cut-off"""
    u = [0x00000000, 0x00000001, 0x00000002, 0x00000123, 0x0007FFFF, 0x00400000, 0x007FFFFF, 0x00800000, 0x00800001,
         0x3F800000, 0x3F7FFFFF, 0x3F800001, 0x7F7FFFFF, 0x7F7FFFFE, 0x7F000000, 0x7F800000, 0x7FC00000, 0x7F800001, 0x7FFFFFFF]
    for c in (2.0 ** 22, 1e9, 2.0 ** 19, np.pi / 2, np.pi, 2 * np.pi):
        b = int(bits(np.float32(c)))
        u += list(range(b - 8, b + 9))
    u = np.array(u, np.uint32)
    return floats(np.concatenate([u, u | np.uint32(0x80000000)]))


def switch_neighbourhood():
    """every f32 within 2^16 ulps of +-2^22, where sin / cos change reduction"""
    b = int(bits(np.float32(2.0 ** 22)))
    u = np.arange(b - (1 << 16), b + (1 << 16), dtype=np.uint32)
    return floats(np.concatenate([u, u | np.uint32(0x80000000)]))


ATAN2_SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, F32_MAX, -F32_MAX, np.inf, -np.inf, np.nan], np.float32)


def atan2_special_pairs():
    """the cross product of ATAN2_SPECIAL with itself: (y, x)"""
    y, x = np.meshgrid(ATAN2_SPECIAL, ATAN2_SPECIAL, indexing="ij")
    return y.ravel().copy(), x.ravel().copy()


def atan2_extreme_pairs():
    """pairs whose ratio y/x overflows or underflows f32 (the f64 ratio of two f32 never does: it stays within 2^+-277),
    and pairs of equal and nearly equal magnitude"""
    big = floats(np.array([0x7F7FFFFF, 0x7F000000, 0x7E800000, 0x60000000], np.uint32))
    small = floats(np.array([0x00000001, 0x00000010, 0x00800000, 0x20000000], np.uint32))
    ys, xs = [], []
    for a in big:
        for b in small:
            for sy in (1, -1):
                for sx in (1, -1):
                    ys += [sy * a, sy * b]
                    xs += [sx * b, sx * a]
    near = floats(np.arange(0x3F7FFFF0, 0x3F800010, dtype=np.uint32))
    for sy in (1, -1):
        for sx in (1, -1):
            ys += list(sy * near)
            xs += list(sx * np.full_like(near, 1.0))
    return np.array(ys, np.float32), np.array(xs, np.float32)


def atan2_random_pairs(n, seed):
    rng = np.random.default_rng(seed)
    return floats(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)), \
        floats(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
