"""ctypes binding of tests/emu/emu_rays.cpp (vk_trace.h trace_ray on the host).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_ffi
from vecchio_amd import ffi
from vecchio_amd.scene import HIT_DTYPE, RAY_DTYPE

_bound = False


def load():
    global _bound
    from vecchio_amd import build
    build.build_emu()                  # (a library built before emu_rays.cpp joined it is stale by its stamp)
    lib = emu_ffi.load()
    if not _bound:
        lib.emu_rays.restype = C.c_int
        lib.emu_rays.argtypes = [C.POINTER(ffi.SceneDesc), C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                 C.POINTER(C.c_uint32)]
        lib.emu_rays_last_error.restype = C.c_char_p
        _bound = True
    return lib


def trace_rays(desc, rays, seed=0, first_index=0):
    """trace_ray for every ray of a RAY_DTYPE array: (HIT_DTYPE array, the linearised scene's features)"""
    lib = load()
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    hits = np.zeros(len(rays), HIT_DTYPE)
    features = C.c_uint32()
    st = lib.emu_rays(desc, seed, first_index, rays.ctypes.data, len(rays), hits.ctypes.data, C.byref(features))
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_rays_last_error().decode()}")
    return hits, features.value
