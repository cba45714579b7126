"""ctypes binding of the non-local-means emulator tests/emu/emu_nlm.cpp: prepare and the filter of every pixel on the host, the kernels'
own per-pixel code (vk_nlm.h through g++).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_paths_ffi

_bound = False


def load():
    global _bound
    lib = emu_paths_ffi.load()
    if not _bound:
        lib.emu_nlm_prepare.restype = C.c_int
        lib.emu_nlm_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
        lib.emu_nlm_filter.restype = C.c_int
        lib.emu_nlm_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float,
                                       C.c_float, C.c_void_p, C.c_void_p]
        lib.emu_nlm_last_error.restype = C.c_char_p
        _bound = True
    return lib


def filter(color, stderr3, albedo=None, R=7, F=3, k=0.45, alpha=1.0, albedo_floor=1e-3, want_stderr=True):
    """tests/nlm_ref.py filter()'s twin in C++: (H, W, 3) float32 images, y up -> (out, stderr3_out or None)"""
    lib = load()
    color = np.ascontiguousarray(color, np.float32)
    stderr3 = np.ascontiguousarray(stderr3, np.float32)
    alb = None if albedo is None else np.ascontiguousarray(albedo, np.float32)
    H, W = color.shape[:2]
    out = np.full((H, W, 3), 7.0, np.float32)
    se = np.full((H, W, 3), 7.0, np.float32) if want_stderr else None
    st = lib.emu_nlm_filter(color.ctypes.data, stderr3.ctypes.data, None if alb is None else alb.ctypes.data, W, H, R, F,
                            float(np.float32(k)), float(np.float32(alpha)), float(np.float32(albedo_floor)), out.ctypes.data,
                            None if se is None else se.ctypes.data)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_nlm_last_error().decode()}")
    return out, se
