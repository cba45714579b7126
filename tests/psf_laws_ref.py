"""The f64 laws of the point-spread stage and the error bounds they are held to.  The yardsticks share no code with the operator: a direct
f64 convolution and numpy.fft in f64.  TESTS ONLY.

The bounds, from the arithmetic.  u = 2^-24 is f32's unit roundoff; gamma_n = n u / (1 - n u).

  One butterfly stage.  Higham, "Accuracy and Stability of Numerical Algorithms" (2nd ed.), Theorem 24.2: a radix-2 transform of length
  2^m whose twiddles carry an absolute error of at most mu computes y^ with ||y^ - y||_2 <= (m eta / (1 - m eta)) ||y||_2, eta = mu +
  gamma_4 (sqrt(2) + mu): the transform is a product of m sparse factors of 2-norm sqrt(2), each applied with a complex multiply (two
  products and an addition per component: gamma_2, sqrt(2) gamma_2 as a complex relative error, Lemma 3.5) and an addition.  The tables
  are f64 values within 2^-50 of the truth (eleven f64 products and a half-angle chain) rounded to f32 componentwise, so mu <= u (1 +
  2^-20).  Negating w.im is exact, so the inverse has the same bound.
  Two dimensions.  Rows then columns are m = m_x + m_y such factors in a row, so E = m eta / (1 - m eta) bounds the 2-D transform's
  relative error in the Frobenius norm.  An unscaled 2-D transform has norm sqrt(N2), N2 = Px Py.
  The chain.  With b the padded bright part (||b||_2 = b2) and k one channel of the normalised kernel (||k||_2 = k2, sum S):
    ||F^ - F||_2 <= E sqrt(N2) b2 =: dF                       ||F||_2 = sqrt(N2) b2 =: F2
    max |G^ - G| <= ||G^ - G||_2 <= E sqrt(N2) k2 =: dG       max |G| <= S, so max |G^| <= S + dG =: Gm
    product (complex relative error p = sqrt(2) gamma_2):      ||P^ - P||_2 <= dF Gm + F2 dG + p (F2 + dF) Gm =: dP
                                                               ||P^||_2 <= (F2 + dF) Gm (1 + p) =: P2
    inverse, unscaled:                                         ||c^ N2 - c N2||_2 <= sqrt(N2) dP + E sqrt(N2) P2
    the multiplication by 1 / N2 is exact (a power of two; no result here is near the subnormal range).
  So every pixel of C is within dC = (dP + E P2) / sqrt(N2) of the exact linear convolution of b with the f32 kernel k: the 2-norm of the
  error bounds each of its entries.  This is loose by about sqrt(N2) (the error of G is spread over N2 entries, not gathered in one);
  DESIGN.md records the measured deviations next to it.  The bound is not tuned to them.
  Composite.  out = fl(I + fl(s fl(C^ - B))): three roundings, so |out - (I + s (C - B))| <= s dC (1 + 3u) + 3.01 u (|I| + s (|C| + |B|)).
  numpy.fft in f64 carries the same kind of error with u = 2^-53: 1e-12 (|I| + |C| + |B|) covers it with room.
"""
import math

import numpy as np

import psf_ref

u = 2.0 ** -24


def gamma(n):
    return n * u / (1.0 - n * u)


def transform_error(Px, Py):
    """E: the relative Frobenius-norm error of one 2-D transform"""
    m = (Px.bit_length() - 1) + (Py.bit_length() - 1)
    mu = u * (1.0 + 2.0 ** -20)
    eta = mu + gamma(4) * (math.sqrt(2.0) + mu)
    return m * eta / (1.0 - m * eta)


def roundtrip_bound(Px, Py, a):
    """max |IFFT2(FFT2(a)) - a| of a (Py, Px, 2) array: forward E ||a||, then the inverse of what came out: E ||a|| (1 + E)"""
    E = transform_error(Px, Py)
    return (E + E * (1.0 + E)) * float(np.sqrt((np.asarray(a, np.float64) ** 2).sum()))


def conv_bound(W, H, kn, B):
    """dC per channel, (3,): kn the normalised (K, K, 3) f32 kernel, B the (H, W, 3) bright part"""
    K = kn.shape[0]
    Px, Py = psf_ref.padded(W, H, K)
    N2 = float(Px) * float(Py)
    E = transform_error(Px, Py)
    p = math.sqrt(2.0) * gamma(2)
    out = np.zeros(3)
    for c in range(3):
        b2 = float(np.sqrt((B[..., c].astype(np.float64) ** 2).sum()))
        k = kn[..., c].astype(np.float64)
        k2, S = float(np.sqrt((k ** 2).sum())), float(k.sum())
        dF, F2 = E * math.sqrt(N2) * b2, math.sqrt(N2) * b2
        dG = E * math.sqrt(N2) * k2
        Gm = S + dG
        dP = dF * Gm + F2 * dG + p * (F2 + dF) * Gm
        P2 = (F2 + dF) * Gm * (1.0 + p)
        out[c] = (dP + E * P2) / math.sqrt(N2)
    return out


def out_bound(I, kn, B, C, s):
    """elementwise bound on |out - (I + s (C - B))|, (H, W, 3); C the exact convolution"""
    H, W = I.shape[:2]
    dC = conv_bound(W, H, kn, B)
    I64 = np.abs(np.asarray(I, np.float64))
    return s * dC[None, None, :] * (1.0 + 3.0 * u) + 3.01 * u * (I64 + s * (np.abs(C) + np.abs(B))) + 1e-12 * (I64 + np.abs(C) + np.abs(B))


def conv_direct(B, kn, period=None):
    """the exact convolution in f64 by its definition, tap by tap: C(x, y) = sum B(x - dx, y - dy) k(r + dx, r + dy); zero outside the
    frame, or, with period=True, the frame repeated with period W x H (the circular convolution a wrap-around would give)"""
    H, W = B.shape[:2]
    K = kn.shape[0]
    r = (K - 1) // 2
    B64, k64 = B.astype(np.float64), kn.astype(np.float64)
    C = np.zeros((H, W, 3))
    if period:
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                C += np.roll(B64, (dy, dx), axis=(0, 1)) * k64[r + dy, r + dx]
        return C
    pad = np.zeros((H + 2 * r, W + 2 * r, 3))
    pad[r:r + H, r:r + W] = B64
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            C += pad[r - dy:r - dy + H, r - dx:r - dx + W] * k64[r + dy, r + dx]
    return C


def conv_numpy_fft(B, kn):
    """the same by numpy.fft in f64, zero-padded to W + K - 1 by H + K - 1 (no power of two needed: another code path entirely)"""
    H, W = B.shape[:2]
    K = kn.shape[0]
    r = (K - 1) // 2
    sy, sx = H + K - 1, W + K - 1
    C = np.zeros((H, W, 3))
    for c in range(3):
        full = np.fft.irfft2(np.fft.rfft2(B[..., c].astype(np.float64), (sy, sx)) * np.fft.rfft2(kn[..., c].astype(np.float64), (sy, sx)), (sy, sx))
        C[..., c] = full[r:r + H, r:r + W]
    return C


def positive_frame(W, H, seed):
    """finite, positive, below 2^20: the bright part is the frame itself when threshold = 0"""
    rng = np.random.default_rng(seed)
    I = np.exp2(rng.uniform(-6, 6, (H, W, 3))).astype(np.float32)
    flat = I.reshape(-1, 3)
    for i in rng.integers(0, W * H, max(1, W * H // 40)):
        flat[i] = np.float32(rng.uniform(50, 3000))
    return I


def random_kernel(K, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, 1, (K, K, 3)) ** 4).astype(np.float32)


def worst(got, want, bound):
    """the largest |got - want| / bound over the frame: a law holds when it is <= 1"""
    d = np.abs(np.asarray(got, np.float64) - want)
    return float((d / bound).max()), float(d.max()), float(bound.max())


# ---- the laws, over any `apply(I, kernel, strength, threshold) -> out`.  Each returns the figures it checked, for the record. ----------

LAW_SHAPES = [(24, 20, 9), (37, 11, 5), (60, 33, 17)]


def law_a(apply, W, H, K, seed, s=0.6):
    """against the direct f64 convolution and against numpy.fft in f64, on a random frame and kernel"""
    I, k = positive_frame(W, H, seed), random_kernel(K, seed + 1)
    kn = psf_ref.normalise(k)
    out = apply(I, k, s, 0.0)
    fig = {}
    for name, C in (("direct", conv_direct(I, kn)), ("numpy.fft", conv_numpy_fft(I, kn))):
        want = I.astype(np.float64) + s * (C - I)
        fig[name] = worst(out, want, out_bound(I, kn, I, C, s))
        assert fig[name][0] <= 1.0, (name, fig[name])
    return fig


def law_b(apply, W, H, K, seed):
    """a delta kernel gives out ~ I"""
    I = positive_frame(W, H, seed)
    k = np.zeros((K, K, 3), np.float32)
    k[(K - 1) // 2, (K - 1) // 2] = 3.0
    kn = psf_ref.normalise(k)
    out = apply(I, k, 1.0, 0.0)
    fig = worst(out, I.astype(np.float64), out_bound(I, kn, I, I.astype(np.float64), 1.0))
    assert fig[0] <= 1.0, fig
    return fig


def law_c(apply, W, H, K, seed, s=0.5, v=100.0):
    """one interior impulse gives strength * k placed there, and sum(out) = sum(I) within the bound"""
    r = (K - 1) // 2
    assert W > 2 * r and H > 2 * r
    k = random_kernel(K, seed)
    kn = psf_ref.normalise(k)
    x0, y0 = r + (W - 2 * r) // 2, r + (H - 2 * r) // 3
    I = np.zeros((H, W, 3), np.float32)
    I[y0, x0] = v
    out = apply(I, k, s, 0.0)
    want = I.astype(np.float64).copy()
    want[y0, x0] -= s * v
    want[y0 - r:y0 + r + 1, x0 - r:x0 + r + 1] += s * v * kn.astype(np.float64)
    bound = out_bound(I, kn, I, (want - I + s * I) / s, s)
    fig = worst(out, want, bound)
    assert fig[0] <= 1.0, fig
    S = kn.astype(np.float64).sum(axis=(0, 1))
    total = np.abs(out.astype(np.float64).sum(axis=(0, 1)) - (I.astype(np.float64).sum(axis=(0, 1)) + s * v * (S - 1.0)))
    assert (total <= bound.sum(axis=(0, 1))).all(), (total, bound.sum(axis=(0, 1)))
    return fig


def law_d(apply, W, H, K, s=1.0, v=1000.0):
    """no wrap-around: an impulse in each corner, a kernel with its mass at its far corners.  What leaves the frame is lost: the result is
    the linear convolution, and where that gives nothing nothing arrives beyond the bound.  Power: a circular convolution of period W x H
    differs from the result by orders of magnitude more than the bound."""
    r = (K - 1) // 2
    assert W > 4 * r and H > 4 * r
    k = np.zeros((K, K, 3), np.float32)
    for ky, kx in ((0, 0), (0, K - 1), (K - 1, 0), (K - 1, K - 1)):
        k[ky, kx] = (1.0, 2.0, 3.0)
    k[r, r] = 1.0
    kn = psf_ref.normalise(k)
    I = np.zeros((H, W, 3), np.float32)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        I[y, x] = v
    out = apply(I, k, s, 0.0)
    lin, circ = conv_direct(I, kn), conv_direct(I, kn, period=True)
    want = I.astype(np.float64) + s * (lin - I)
    bound = out_bound(I, kn, I, lin, s)
    fig = worst(out, want, bound)
    assert fig[0] <= 1.0, fig
    empty = (lin == 0) & (I == 0)
    wrapped = empty & (circ > 0)
    assert wrapped.sum() == 4 * 3 * 3               # each corner's three far taps would come back in through the opposite edges
    assert (np.abs(out[empty]) <= bound[empty]).all()
    power = np.abs(out.astype(np.float64) - (I + s * (circ - I)))[wrapped].min() / bound.max()
    # (what a wrap would bring is s v k(corner) >= 1000 / 5; the bound is about v (E + dG) with dG = E sqrt(N2) k2, a few 1e-4 v at
    # these sizes: between two and three orders of magnitude, so two are asked for)
    assert power > 1e2, power
    return fig + (float(power),)


def law_e(apply, W, H, K, seed, s=0.7):
    """three different channel kernels act independently: channel c is what the kernel (k_c, k_c, k_c) gives in channel c, exactly, and
    does not depend on the other channels of the frame"""
    I, k = positive_frame(W, H, seed), random_kernel(K, seed + 1)
    assert not np.array_equal(k[..., 0], k[..., 1]) and not np.array_equal(k[..., 1], k[..., 2])
    out = apply(I, k, s, 0.0)
    for c in range(3):
        same = apply(I, np.repeat(k[..., c:c + 1], 3, axis=2), s, 0.0)
        assert np.array_equal(same[..., c], out[..., c]), c
        alone = np.zeros_like(I)
        alone[..., c] = I[..., c]
        got = apply(alone, k, s, 0.0)
        assert np.array_equal(got[..., c], out[..., c]), c
        others = [d for d in range(3) if d != c]
        assert (got[..., others] == 0).all()
    return ()


def law_f(apply, W, H, K, seed):
    """linearity in strength: out(s) - I = s (out(1) - I) within the roundings of the composite alone.  With d = fl(C^ - B), the same
    bits for every s: out(1) = (I + d)(1 + e1), out(s) = (I + s d (1 + e2))(1 + e3), |e| <= u, so the difference is at most
    u ((1 + s) |I| + 3.01 s |d|), and |d| <= |out(1)| (1 + 2u) + |I|."""
    I, k = positive_frame(W, H, seed), random_kernel(K, seed + 1)
    one = apply(I, k, 1.0, 0.0).astype(np.float64)
    I64 = I.astype(np.float64)
    worst_ratio = 0.0
    for s in (0.0, 0.125, 0.3, 0.77):
        out = apply(I, k, s, 0.0).astype(np.float64)
        s32 = float(np.float32(s))
        bound = u * ((1.0 + s32) * np.abs(I64) + 3.01 * s32 * (np.abs(one) * (1.0 + 2.0 * u) + np.abs(I64)))
        d = np.abs(out - (I64 + s32 * (one - I64)))
        if s == 0.0:
            assert np.array_equal(out, I64)
        else:
            worst_ratio = max(worst_ratio, float((d / bound).max()))
    assert worst_ratio <= 1.0, worst_ratio
    return (worst_ratio,)


def run_all(apply):
    """every law on every shape; the figures by law"""
    fig = {}
    for i, (W, H, K) in enumerate(LAW_SHAPES):
        fig[("a", W, H, K)] = law_a(apply, W, H, K, 10 + i)
        fig[("b", W, H, K)] = law_b(apply, W, H, K, 20 + i)
        fig[("c", W, H, K)] = law_c(apply, W, H, K, 30 + i)
        fig[("e", W, H, K)] = law_e(apply, W, H, K, 40 + i)
        fig[("f", W, H, K)] = law_f(apply, W, H, K, 50 + i)
    for W, H, K in ((24, 20, 9), (30, 21, 7)):
        fig[("d", W, H, K)] = law_d(apply, W, H, K)
    return fig
