"""The point-spread stage on the CPU: the host build of vk_psf.h (tests/emu/emu_psf.cpp: the kernels' own per-element code through g++)
against the numpy restatement tests/psf_ref.py, bit for bit as floats (-0 equal to +0, a NaN's payload aside) over tests/psf_cases.py;
the twiddle tables of every N = 2 .. 4096 against the restatement's, bit for bit, with T[0] = (1, 0) and T[N/4] = (0, -1) exactly; the
kernel's normalisation and what a load refuses; the bare transform."""
import numpy as np
import pytest

import emu_psf_ffi as EMU
import psf_cases as PC
import psf_ref as R

f32 = np.float32


@pytest.mark.parametrize("name", [c[0] for c in PC.CASES])
def test_host_build_equals_the_restatement(name, emu):
    I, k, st, th = PC.inputs(name)
    want = R.apply(I, k, st, th)
    got = EMU.apply(I, k, st, th)
    assert R.same_floats(got, want), name
    _, W, H, K, _, _, _, special = PC.case(name)
    assert got.shape == (H, W, 3)
    fin = np.isfinite(I)
    assert np.array_equal(np.isfinite(got), fin)                         # a component that is not finite stays what it was
    assert np.array_equal(got[~fin & ~np.isnan(I)], I[~fin & ~np.isnan(I)]) and np.isnan(got[np.isnan(I)]).all()
    if st == 0.0:
        assert R.same_floats(got, I)
    else:
        assert not R.same_floats(got, I)


def test_twiddle_tables_of_every_length(emu):
    N = 2
    while N <= 4096:
        T, want = EMU.twiddles(N), R.twiddles(N)
        assert T.shape == (N // 2, 2) and np.array_equal(T.view(np.uint32), want.view(np.uint32)), N
        assert T[0].view(np.uint32).tolist() == [0x3F800000, 0]          # (1, +0)
        if N >= 4:
            assert T[N // 4].view(np.uint32).tolist() == [0, 0xBF800000]                 # (+0, -1)
        # exp(-2 pi i k / N) to f32 rounding: half an ulp of a value below 1, and the f64 chain's error far below that
        k = np.arange(N // 2)
        exact = np.exp(-2j * np.pi * k / N)
        assert np.abs(T[:, 0] - exact.real).max() <= 2.0 ** -24 * (1 + 2.0 ** -20)
        assert np.abs(T[:, 1] - exact.imag).max() <= 2.0 ** -24 * (1 + 2.0 ** -20)
        N *= 2


def test_a_shorter_table_is_every_other_entry_of_the_longer_one(emu):
    """the rule depends on k / N alone: T_N[k] == T_2N[2k], bit for bit"""
    big = EMU.twiddles(4096)
    N = 2048
    while N >= 2:
        assert np.array_equal(EMU.twiddles(N).view(np.uint32), big[::4096 // N].view(np.uint32)), N
        N //= 2


def test_normalisation_and_what_a_load_refuses(emu):
    k = PC.kernel(9, 3)
    got, want = EMU.normalise(k), R.normalise(k)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    S = got.astype(np.float64).sum(axis=(0, 1))
    assert (np.abs(S - 1.0) <= 81 * 2.0 ** -24).all()                  # every tap rounded once, half an ulp of a value below 1
    for bad, word in ((np.nan, "not finite"), (np.inf, "not finite"), (-1e-30, "negative")):
        kb = k.copy()
        kb[2, 7, 1] = bad
        for fn in (EMU.normalise, R.normalise):
            with pytest.raises(ValueError, match=word):
                fn(kb)
    kb = k.copy()
    kb[..., 2] = 0
    for fn in (EMU.normalise, R.normalise):
        with pytest.raises(ValueError, match="sums to nothing"):
            fn(kb)


@pytest.mark.parametrize("size", [(2, 2), (8, 2), (2, 16), (64, 32), (4096, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_bare_transform(size, emu):
    Px, Py = size
    a = np.random.default_rng(Px + Py).normal(0, 1, (Py, Px, 2)).astype(f32)
    fr, fi = R.fft2(a[..., 0], a[..., 1])
    assert R.same_floats(EMU.fft2(a), np.stack([fr, fi], axis=-1))
    br, bi = R.fft2(fr, fi, inverse=True)
    assert R.same_floats(EMU.fft2(np.stack([fr, fi], axis=-1), inverse=True), np.stack([br, bi], axis=-1))
    # and it is the transform: numpy's in f64
    want = np.fft.fft2(a[..., 0].astype(np.float64) + 1j * a[..., 1])
    import psf_laws_ref as L
    norm = float(np.sqrt((a.astype(np.float64) ** 2).sum()))
    assert np.abs((fr + 1j * fi) - want).max() <= L.transform_error(Px, Py) * np.sqrt(Px * Py) * norm
