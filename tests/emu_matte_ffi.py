"""ctypes binding of tests/emu/emu_matte.cpp (vk_matte.h matte_sample, matte_insert and matte_sort on the host).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_ffi
from vecchio_amd import ffi

_bound = False


def load():
    global _bound
    from vecchio_amd import build
    build.build_emu()                  # (a library built before emu_matte.cpp joined it is stale by its stamp)
    lib = emu_ffi.load()
    if not _bound:
        lib.emu_matte.restype = C.c_int
        lib.emu_matte.argtypes = [C.POINTER(ffi.SceneDesc), C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_uint32, C.c_uint32,
                                  C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        lib.emu_matte_table.restype = C.c_int
        lib.emu_matte_table.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        lib.emu_matte_last_error.restype = C.c_char_p
        _bound = True
    return lib


def _check(lib, st):
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_matte_last_error().decode()}")


def matte_samples(desc, cam, p, first_sample, n, kind):
    """matte_sample of samples first_sample .. first_sample + n - 1 of every pixel of the call's partition: (height, width, n) uint32
    (0xDEADBEEF outside the partition), and the linearised scene's features"""
    lib = load()
    ids = np.full((p.height, p.width, n), 0xDEADBEEF, np.uint32)
    features = C.c_uint32()
    _check(lib, lib.emu_matte(desc, C.byref(cam), C.byref(p), first_sample, n, kind, 1, 0, ids.ctypes.data, None, None, C.byref(features)))
    return ids, features.value


def matte_window(desc, cam, p, first_sample, n, kind, ranks):
    """the window's table in matte_kernel's order: ids, counts (height, width, ranks), overflow (height, width)"""
    lib = load()
    ids = np.full((p.height, p.width, ranks), 0xDEADBEEF, np.uint32)
    counts = np.full((p.height, p.width, ranks), 0xDEADBEEF, np.uint32)
    overflow = np.full((p.height, p.width), 0xDEADBEEF, np.uint32)
    _check(lib, lib.emu_matte(desc, C.byref(cam), C.byref(p), first_sample, n, kind, ranks, 1, ids.ctypes.data, counts.ctypes.data,
                              overflow.ctypes.data, None))
    return ids, counts, overflow


def table(sample_ids, ranks):
    """matte_insert and matte_sort on one pixel's ids, in order: (ids, counts, overflow)"""
    lib = load()
    sample_ids = np.ascontiguousarray(sample_ids, np.uint32)
    ids, counts, over = np.zeros(ranks, np.uint32), np.zeros(ranks, np.uint32), C.c_uint32()
    _check(lib, lib.emu_matte_table(sample_ids.ctypes.data, len(sample_ids), ranks, ids.ctypes.data, counts.ctypes.data, C.byref(over)))
    return ids, counts, over.value
