"""ctypes binding of the point-spread emulator tests/emu/emu_psf.cpp: the whole operator on the host from the kernels' own per-element
code (vk_psf.h through g++), and the library's twiddle tables, normalisation and bare transform.  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_paths_ffi

_bound = False


def load():
    global _bound
    lib = emu_paths_ffi.load()
    if not _bound:
        lib.emu_psf_apply.restype = C.c_int
        lib.emu_psf_apply.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
        lib.emu_psf_twiddles.restype = C.c_int
        lib.emu_psf_twiddles.argtypes = [C.c_uint32, C.c_void_p]
        lib.emu_psf_normalise.restype = C.c_int
        lib.emu_psf_normalise.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
        lib.emu_psf_fft2.restype = C.c_int
        lib.emu_psf_fft2.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.emu_psf_last_error.restype = C.c_char_p
        _bound = True
    return lib


def apply(I, kernel, strength=0.15, threshold=0.0):
    """tests/psf_ref.py apply()'s twin in C++: an (H, W, 3) float32 frame, y up, and a (K, K, 3) kernel -> the frame's shape"""
    lib = load()
    I = np.ascontiguousarray(I, np.float32)
    kernel = np.ascontiguousarray(kernel, np.float32)
    H, W = I.shape[:2]
    out = np.full((H, W, 3), 7.0, np.float32)
    st = lib.emu_psf_apply(I.ctypes.data, W, H, kernel.shape[0], kernel.ctypes.data, float(np.float32(strength)),
                           float(np.float32(threshold)), out.ctypes.data)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_psf_last_error().decode()}")
    return out


def twiddles(N):
    """(N / 2, 2) float32: (re, im)"""
    T = np.zeros((N // 2, 2), np.float32)
    assert load().emu_psf_twiddles(N, T.ctypes.data) == 0
    return T


def normalise(kernel):
    kernel = np.ascontiguousarray(kernel, np.float32)
    out = np.zeros_like(kernel)
    lib = load()
    if lib.emu_psf_normalise(kernel.shape[0], kernel.ctypes.data, out.ctypes.data) != 0:
        raise ValueError(lib.emu_psf_last_error().decode())
    return out


def fft2(a, inverse=False):
    """(Py, Px, 2) float32 -> the same shape"""
    a = np.array(a, np.float32, order="C")
    assert load().emu_psf_fft2(a.shape[1], a.shape[0], 1 if inverse else 0, a.ctypes.data) == 0
    return a
