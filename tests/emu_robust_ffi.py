"""ctypes binding of the robust-film emulator tests/emu/emu_robust.cpp: vk_robust_resolve's per-pixel arithmetic on the host, the
kernel's own (vk_robust.h robust_resolve_pixel<K> through g++).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_paths_ffi

_bound = False


def load():
    global _bound
    lib = emu_paths_ffi.load()
    if not _bound:
        lib.emu_robust_resolve.restype = C.c_int
        lib.emu_robust_resolve.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.emu_robust_last_error.restype = C.c_char_p
        _bound = True
    return lib


def resolve(state, mode, trim=0):
    """tests/robust_ref.py resolve()'s twin in C++: state (..., K, 4) int64 -> (rgb (..., 3), stderr (..., 3)) float32"""
    lib = load()
    state = np.ascontiguousarray(state, np.int64)
    K, shape = state.shape[-2], state.shape[:-2]
    n = int(np.prod(shape, dtype=np.int64))
    rgb, se = np.full(shape + (3,), 7, np.float32), np.full(shape + (3,), 7, np.float32)
    st = lib.emu_robust_resolve(K, state.ctypes.data, n, mode, trim, rgb.ctypes.data, se.ctypes.data)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_robust_last_error().decode()}")
    return rgb, se
