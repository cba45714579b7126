"""ctypes binding of tests/emu/emu_radiance.cpp (vk_trace.h radiance_sample on the host).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_ffi
from vecchio_amd import ffi
from vecchio_amd.scene import KEY_DTYPE, RAY_DTYPE, DeviceScene

_bound = False


def load():
    global _bound
    from vecchio_amd import build
    build.build_emu()                  # (a library built before emu_radiance.cpp joined it is stale by its stamp)
    lib = emu_ffi.load()
    if not _bound:
        lib.emu_radiance.restype = C.c_int
        lib.emu_radiance.argtypes = [C.POINTER(ffi.SceneDesc), C.POINTER(ffi.RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p,
                                     C.c_void_p, C.POINTER(C.c_uint32)]
        lib.emu_radiance_last_error.restype = C.c_char_p
        _bound = True
    return lib


def radiance_samples(desc, rays, keys=None, **params):
    """what DeviceScene.debug_radiance_samples returns, computed on the host: (n, samples_per_ray, 4) float32 — rgb and the final
    counter of every sample — and the linearised scene's features"""
    lib = load()
    rp = DeviceScene.radiance_params(**params)
    rays = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
    n = len(rays)
    if keys is not None:
        keys = np.ascontiguousarray(keys, KEY_DTYPE).reshape(-1)
        assert len(keys) == n
    out = np.zeros((n, rp.samples_per_ray, 4), np.float32)
    features = C.c_uint32()
    st = lib.emu_radiance(desc, C.byref(rp), rays.ctypes.data, n, keys.ctypes.data if keys is not None else None, out.ctypes.data,
                          C.byref(features))
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_radiance_last_error().decode()}")
    return out, features.value
