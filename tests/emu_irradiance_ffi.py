"""ctypes binding of tests/emu/emu_irradiance.cpp (vk_trace.h irradiance_sample on the host).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_ffi
from vecchio_amd import ffi
from vecchio_amd.scene import RAY_DTYPE, DeviceScene

_bound = False


def load():
    global _bound
    from vecchio_amd import build
    build.build_emu()                  # (a library built before emu_irradiance.cpp joined it is stale by its stamp)
    lib = emu_ffi.load()
    if not _bound:
        lib.emu_irradiance.restype = C.c_int
        lib.emu_irradiance.argtypes = [C.POINTER(ffi.SceneDesc), C.POINTER(ffi.RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p,
                                       C.c_void_p, C.POINTER(C.c_uint32)]
        lib.emu_irradiance_last_error.restype = C.c_char_p
        _bound = True
    return lib


def irradiance_samples(desc, points, **params):
    """what DeviceScene.debug_irradiance_samples returns, computed on the host: (samples (n, samples_per_ray, 4) float32 — rgb and the
    final counter of every sample —, dirs (n, samples_per_ray, 4) float32 — the direction drawn for it, then 0)"""
    lib = load()
    rp = DeviceScene.radiance_params(**params)
    points = np.ascontiguousarray(points, RAY_DTYPE).reshape(-1)
    n = len(points)
    samples = np.zeros((n, rp.samples_per_ray, 4), np.float32)
    dirs = np.zeros((n, rp.samples_per_ray, 4), np.float32)
    st = lib.emu_irradiance(desc, C.byref(rp), points.ctypes.data, n, samples.ctypes.data, dirs.ctypes.data, None)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_irradiance_last_error().decode()}")
    return samples, dirs
