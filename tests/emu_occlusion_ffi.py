"""ctypes binding of tests/emu/emu_occlusion.cpp (vk_trace.h occluded_ray on the host).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_ffi
from vecchio_amd import ffi
from vecchio_amd.scene import RAY_DTYPE

_bound = False


def load():
    global _bound
    from vecchio_amd import build
    build.build_emu()                  # (a library built before emu_occlusion.cpp joined it is stale by its stamp)
    lib = emu_ffi.load()
    if not _bound:
        lib.emu_occlusion.restype = C.c_int
        lib.emu_occlusion.argtypes = [C.POINTER(ffi.SceneDesc), C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                      C.POINTER(C.c_uint32)]
        lib.emu_occlusion_last_error.restype = C.c_char_p
        _bound = True
    return lib


def trace_occluded(desc, rays, seed=0, first_index=0):
    """occluded_ray for every ray of a RAY_DTYPE array: (uint8 array, the linearised scene's features)"""
    lib = load()
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    out = np.full(len(rays), 0xAA, np.uint8)
    features = C.c_uint32()
    st = lib.emu_occlusion(desc, seed, first_index, rays.ctypes.data, len(rays), out.ctypes.data, C.byref(features))
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_occlusion_last_error().decode()}")
    return out, features.value
