"""ctypes binding of tests/emu/emu_adapt.cpp: the top-up of a film's tile run (vk_adapt_begin) on the host — the kernel's own index code
(vk_adapt.h adapt_locate) and vk_trace.h start_sample_core.  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_paths_ffi
from vecchio_amd import ffi
from vecchio_amd.scene import PATH_STATE_DTYPE, RAY_DTYPE

_bound = False


def load():
    global _bound
    lib = emu_paths_ffi.load()
    if not _bound:
        lib.emu_adapt_total.restype = C.c_int
        lib.emu_adapt_total.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
        lib.emu_adapt_sequence.restype = C.c_int
        lib.emu_adapt_sequence.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p,
                                           C.c_void_p]
        lib.emu_adapt_emit.restype = C.c_int
        lib.emu_adapt_emit.argtypes = [C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64,
                                       C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.emu_adapt_last_error.restype = C.c_char_p
        _bound = True
    return lib


def _check(lib, st):
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_adapt_last_error().decode()}")


def _map(tile_n):
    return np.ascontiguousarray(tile_n, np.uint32).reshape(-1)


def total(width, height, tile_n, n_samples):
    lib = load()
    n = C.c_uint64()
    _check(lib, lib.emu_adapt_total(width, height, _map(tile_n).ctypes.data, n_samples, C.byref(n)))
    return int(n.value)


def sequence(width, height, tile_n, n_samples, samples_done=0, first=0, m=None):
    """(pixel, sample) of paths first .. first + m (default: to the run's end) from adapt_locate"""
    lib = load()
    t = _map(tile_n)
    m = total(width, height, t, n_samples) - first if m is None else m
    pixel, sample = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
    _check(lib, lib.emu_adapt_sequence(width, height, t.ctypes.data, n_samples, samples_done, first, m, pixel.ctypes.data, sample.ctypes.data))
    return pixel, sample


def emit(cam, p, tile_n, n_samples, samples_done=0, first=0, m=None):
    """(rays, states, ids) of paths first .. first + m of the tile run"""
    lib = load()
    t = _map(tile_n)
    m = total(p.width, p.height, t, n_samples) - first if m is None else m
    rays, states, ids = np.zeros(m, RAY_DTYPE), np.zeros(m, PATH_STATE_DTYPE), np.zeros(m, np.uint32)
    _check(lib, lib.emu_adapt_emit(C.byref(cam), C.byref(p), t.ctypes.data, n_samples, samples_done, first, m, rays.ctypes.data,
                                   states.ctypes.data, ids.ctypes.data))
    return rays, states, ids
