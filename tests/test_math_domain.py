"""The shared arithmetic of vecchio_amd/csrc/vk_math.h (sin, cos, sincos, ln, asin, atan2, x^5) over the whole f32 domain, against
the correctly rounded value (tests/math_domain.py correctly_rounded: float64, settled by mpmath near rounding ties).  Oracle,
emulator and device compile this one header, so per-sample parity cannot see an error in it; these tests can.  CPU only.

Coverage, for every unary function: every 61st of the 2^32 bit patterns (~70 M inputs: both signs, subnormals, inf, NaN) and the
special values (signed zeros with the sign of the result, subnormals, FLT_MAX, inf, NaN).  Ranges the render path uses, on top:
  * sin / cos / sincos on [0, 2 pi): every 31st f32 (35 M: all 1.09 G would take minutes of CPU time), and every
    f32 within 2^16 ulps of +-2^22, where the reduction switches from Cody-Waite to Payne-Hanek;
  * asin: every f32 with 1 - 2^-10 <= |x| <= 1, and the NaN domain just beyond;
  * ln: every f32 in [0.5, 2], every f32 in [2^-24, 2^-20) (the smallest 24-bit draws, hittable.rs:473) and every 97th in (0, 2^-24)
    (all 880 M would take minutes).
atan2(y, x): 2^22 random bit-pattern pairs, the cross product of {+-0, +-subnormal, +-1, +-FLT_MAX, +-inf, NaN} against C99 Annex F,
and pairs whose ratio overflows or underflows f32.

The claim held: 0 ulp (correctly rounded) everywhere, and sincosf_ equal to (sinf_, cosf_) bit for bit."""
import os
from concurrent.futures import ThreadPoolExecutor

import mpmath
import numpy as np
import pytest

import math_domain as MD
from math_domain import F32_MAX, correctly_rounded, same

THREADS = max(1, min(8, len(os.sched_getaffinity(0))))      # (ctypes calls and numpy ufuncs release the GIL)


def _check_chunk(oracle, fn, x, y=None):
    """(inputs, misses, undecided) of one chunk: misses = inputs where the host result is not the correctly rounded value"""
    got = oracle.math(MD.OP[fn], x, y)
    und = []
    want = correctly_rounded(fn, x, y, und)
    bad = ~same(got, want)
    return x.size, (x[bad], None if y is None else y[bad], got[bad], want[bad]), und[0]


def check_correctly_rounded(oracle, fn, chunks):
    n = undecided = 0
    misses = []
    with ThreadPoolExecutor(THREADS) as pool:
        for k, (xb, yb, g, w), u in pool.map(lambda c: _check_chunk(oracle, fn, *c) if isinstance(c, tuple) else
                                             _check_chunk(oracle, fn, c), chunks):
            n += k
            undecided += u
            if xb.size:
                misses.append((xb, yb, g, w))
    nmiss = sum(m[0].size for m in misses)
    print(f"{fn}: {n} inputs, {undecided} settled by mpmath, {nmiss} not correctly rounded")
    if nmiss:
        xb, yb, g, w = (np.concatenate([m[i] for m in misses]) if misses[0][i] is not None else None for i in range(4))
        d = np.abs(MD.ulp_index(g) - MD.ulp_index(w))
        ex = [(float(xb[i]),) + (() if yb is None else (float(yb[i]),)) + (float(g[i]), float(w[i])) for i in range(min(5, xb.size))]
        raise AssertionError(f"{fn}: {nmiss} of {n} results not correctly rounded (max {d.max()} ulp), e.g. (args, got, want) {ex}")
    return n


@pytest.mark.parametrize("fn", MD.UNARY)
def test_strided_sweep_of_all_bit_patterns(oracle, fn):
    assert check_correctly_rounded(oracle, fn, MD.sweep_chunks()) == ((1 << 32) + 60) // 61


@pytest.mark.parametrize("fn", MD.UNARY)
def test_special_values(oracle, fn):
    x = MD.specials()
    check_correctly_rounded(oracle, fn, [x])
    got = oracle.math(MD.OP[fn], x)
    z = x == 0
    if fn in ("sin", "asin", "pow5"):                    # odd: f(+-0) = +-0, the sign kept
        assert np.array_equal(MD.bits(got[z]), MD.bits(x[z]))
    if fn == "log":
        assert (got[z] == -np.inf).all() and np.isnan(got[(x < 0) & np.isfinite(x)]).all() and got[x == np.inf][0] == np.inf
    if fn in ("sin", "cos"):
        assert np.isnan(got[np.isinf(x) | np.isnan(x)]).all()
    assert np.isnan(got[np.isnan(x)]).all()


def test_sin_cos_on_the_samplers_range(oracle):
    """[0, 2 pi): the angles of random_cosine_direction, lambertian_random and random_to_sphere (every 31st f32), and the
    neighbourhood of the reduction switch at +-2^22 (every f32)"""
    chunks = list(MD.sampler_angles()) + [MD.switch_neighbourhood()]
    for fn in ("sin", "cos"):
        check_correctly_rounded(oracle, fn, chunks)


def test_large_arguments(oracle):
    """|x| >= 2^22: where the two-constant reduction stopped being exact (up to 2^20 ulps wrong) and |x| >= 1e9 returned 0"""
    x = np.array([1e9, -1e9, 4194304.0, 1.6e7, 1e8, 1e20, -3e30, F32_MAX, -F32_MAX], np.float32)
    with mpmath.workprec(200):
        for fn, f in (("sin", mpmath.sin), ("cos", mpmath.cos)):
            got = oracle.math(MD.OP[fn], x)
            want = np.array([float(f(mpmath.mpf(float(v)))) for v in x], np.float32)
            assert np.array_equal(got, want), (fn, got, want)
    assert oracle.math(0, np.array([1e9], np.float32))[0] == np.float32(0.5458434)


def test_sincos_is_sin_and_cos(oracle):
    """sincosf_ (one reduction for both) equals (sinf_, cosf_) bit for bit; sincosf_small_, the samplers' variant without the
    large-argument branch, equals them on [+0, 2^22)"""
    def chunk(x):
        s, c = oracle.math(0, x), oracle.math(1, x)
        ok = same(oracle.math(11, x), s) & same(oracle.math(12, x), c)
        small = (x >= 0) & (x < 2.0 ** 22) & ~np.signbit(x)
        ok_small = same(oracle.math(13, x[small]), s[small]) & same(oracle.math(14, x[small]), c[small])
        return int((~ok).sum()), int((~ok_small).sum()), int(small.sum())

    chunks = list(MD.sweep_chunks()) + list(MD.sampler_angles()) + \
        [MD.specials(), MD.switch_neighbourhood()]
    with ThreadPoolExecutor(THREADS) as pool:
        res = list(pool.map(chunk, chunks))
    bad, bad_small, n_small = (sum(r[i] for r in res) for i in range(3))
    assert n_small > 50_000_000
    assert bad == 0 and bad_small == 0, (bad, bad_small)


def test_asin_near_one(oracle):
    """every f32 with 1 - 2^-10 <= |x| <= 1 (asin's steepest part: sphere_uv at the poles), and the NaN domain beyond 1"""
    x = MD.asin_near_one()
    assert x.size == 2 * ((1 << 14) + 1)
    check_correctly_rounded(oracle, "asin", [x])
    beyond = np.concatenate(list(MD.range_chunks(np.nextafter(np.float32(1), np.float32(2)), 1.001)))
    assert np.isnan(oracle.math(3, np.concatenate([beyond, -beyond]))).all()


def test_log_ranges(oracle):
    chunks = list(MD.log_ranges())
    assert check_correctly_rounded(oracle, "log", chunks) > (1 << 24) + (1 << 25)


def test_atan2_random_bit_patterns(oracle):
    y, x = MD.atan2_random_pairs(1 << 22, seed=21)
    check_correctly_rounded(oracle, "atan2", [(y[i:i + MD.CHUNK // 4], x[i:i + MD.CHUNK // 4]) for i in range(0, y.size, MD.CHUNK // 4)])


def test_atan2_extreme_ratios(oracle):
    y, x = MD.atan2_extreme_pairs()
    check_correctly_rounded(oracle, "atan2", [(y, x)])


def _annex_f_atan2(y, x):
    """C99 Annex F.9.1.4 atan2(y, x), the f32 result, for y, x in MD.ATAN2_SPECIAL"""
    pi, hpi, qpi = np.float32(np.pi), np.float32(np.pi / 2), np.float32(np.pi / 4)
    if np.isnan(y) or np.isnan(x):
        return np.float32(np.nan)
    sy = -1.0 if np.signbit(y) else 1.0
    if y == 0:
        return np.float32(sy * (pi if np.signbit(x) else 0.0))         # atan2(+-0, -0 or x<0) = +-pi; (+-0, +0 or x>0) = +-0
    if np.isinf(y) and np.isinf(x):
        return np.float32(sy * (3 * np.float64(np.pi) / 4 if x < 0 else qpi))
    if np.isinf(y):
        return np.float32(sy * hpi)
    if x == 0:
        return np.float32(sy * hpi)
    if np.isinf(x):
        return np.float32(sy * (pi if x < 0 else 0.0))
    return None                                                         # finite nonzero: the reference decides


def test_atan2_special_pairs_c99_annex_f(oracle):
    y, x = MD.atan2_special_pairs()
    got = oracle.math(4, y, x)
    cr = correctly_rounded("atan2", y, x)
    for i in range(y.size):
        want = _annex_f_atan2(y[i], x[i])
        if want is None:
            want = cr[i]
        else:      # (the Annex F values rounded once: pi, pi/2, pi/4 and 3 pi/4 in f32)
            assert same(want, cr[i]), (y[i], x[i], want, cr[i])
        assert same(got[i], want), f"atan2({y[i]!r}, {x[i]!r}) = {got[i]!r}, want {want!r}"


def test_reference_helper_against_mpmath():
    """correctly_rounded itself, on 3000 random bit patterns per function, against mpmath alone; and its tie handling on
    exact ties (x^5 of small odd integers: 29^5 has 25 significant bits)"""
    rng = np.random.default_rng(5)
    with mpmath.workprec(200):
        for fn in MD.UNARY + ("atan2",):
            x = MD.floats(rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32))
            y = MD.floats(rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32)) if fn == "atan2" else None
            got = correctly_rounded(fn, x, y)
            for i in range(x.size):
                if not (np.isfinite(x[i]) and (y is None or np.isfinite(y[i]))):
                    continue
                if fn == "log" and x[i] <= 0 or fn == "asin" and abs(x[i]) > 1:
                    continue
                want = MD._mp_round_f32(MD._mp_value(fn, x[i], None if y is None else y[i]))
                assert same(got[i], want), (fn, x[i], None if y is None else y[i], got[i], want)
    odd = np.arange(17, 33, 2, dtype=np.float32)
    und = []
    got = correctly_rounded("pow5", odd, undecided_out=und)
    exact = [int(v) ** 5 for v in odd]
    assert [int(g) for g in got] == [int(np.float32(e)) for e in exact]     # numpy's int -> f32 conversion rounds ties to even
