"""ctypes binding of the query emulators tests/emu/emu_{rays,occlusion,radiance,irradiance}.cpp (vk_trace.h trace_ray, occluded_ray,
radiance_sample and irradiance_sample on the host).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_ffi
from vecchio_amd import ffi
from vecchio_amd.scene import HIT_DTYPE, KEY_DTYPE, RAY_DTYPE, DeviceScene

_bound = False


def load():
    global _bound
    from vecchio_amd import build
    build.build_emu()                  # (a library built before one of the emulators joined it is stale by its stamp)
    lib = emu_ffi.load()
    if not _bound:
        walk = [C.POINTER(ffi.SceneDesc), C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32)]
        paths = [C.POINTER(ffi.SceneDesc), C.POINTER(ffi.RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                 C.POINTER(C.c_uint32)]
        for name, argtypes in (("emu_rays", walk), ("emu_occlusion", walk), ("emu_radiance", paths), ("emu_irradiance", paths)):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = argtypes
            getattr(lib, name + "_last_error").restype = C.c_char_p
        _bound = True
    return lib


def _call(name, *args):
    lib = load()
    st = getattr(lib, name)(*args)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {getattr(lib, name + '_last_error')().decode()}")


def trace_rays(desc, rays, seed=0, first_index=0):
    """trace_ray for every ray of a RAY_DTYPE array: (HIT_DTYPE array, the linearised scene's features)"""
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    hits = np.zeros(len(rays), HIT_DTYPE)
    features = C.c_uint32()
    _call("emu_rays", desc, seed, first_index, rays.ctypes.data, len(rays), hits.ctypes.data, C.byref(features))
    return hits, features.value


def trace_occluded(desc, rays, seed=0, first_index=0):
    """occluded_ray for every ray of a RAY_DTYPE array: (uint8 array, the linearised scene's features)"""
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    out = np.full(len(rays), 0xAA, np.uint8)
    features = C.c_uint32()
    _call("emu_occlusion", desc, seed, first_index, rays.ctypes.data, len(rays), out.ctypes.data, C.byref(features))
    return out, features.value


def radiance_samples(desc, rays, keys=None, **params):
    """what DeviceScene.debug_radiance_samples returns, computed on the host: (n, samples_per_ray, 4) float32 — rgb and the final
    counter of every sample — and the linearised scene's features"""
    rp = DeviceScene.radiance_params(**params)
    rays = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
    n = len(rays)
    if keys is not None:
        keys = np.ascontiguousarray(keys, KEY_DTYPE).reshape(-1)
        assert len(keys) == n
    out = np.zeros((n, rp.samples_per_ray, 4), np.float32)
    features = C.c_uint32()
    _call("emu_radiance", desc, C.byref(rp), rays.ctypes.data, n, keys.ctypes.data if keys is not None else None, out.ctypes.data,
          C.byref(features))
    return out, features.value


def irradiance_samples(desc, points, **params):
    """what DeviceScene.debug_irradiance_samples returns, computed on the host: (samples (n, samples_per_ray, 4) float32 — rgb and the
    final counter of every sample —, dirs (n, samples_per_ray, 4) float32 — the direction drawn for it, then 0)"""
    rp = DeviceScene.radiance_params(**params)
    points = np.ascontiguousarray(points, RAY_DTYPE).reshape(-1)
    n = len(points)
    samples = np.zeros((n, rp.samples_per_ray, 4), np.float32)
    dirs = np.zeros((n, rp.samples_per_ray, 4), np.float32)
    _call("emu_irradiance", desc, C.byref(rp), points.ctypes.data, n, samples.ctypes.data, dirs.ctypes.data, None)
    return samples, dirs
