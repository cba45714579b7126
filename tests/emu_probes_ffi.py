"""ctypes binding of the probe emulator tests/emu/emu_probes.cpp (vk_trace.h probe_sample and sh9 on the host).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_queries_ffi
from vecchio_amd import ffi
from vecchio_amd.scene import RAY_DTYPE, DeviceScene

_bound = False


def load():
    global _bound
    lib = emu_queries_ffi.load()
    if not _bound:
        lib.emu_probes.restype = C.c_int
        lib.emu_probes.argtypes = [C.POINTER(ffi.SceneDesc), C.POINTER(ffi.RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.POINTER(C.c_uint32)]
        lib.emu_probes_last_error.restype = C.c_char_p
        _bound = True
    return lib


def probe_samples(desc, probes, **params):
    """what DeviceScene.debug_probe_samples returns, computed on the host, and the basis values: (samples (n, samples_per_ray, 4) float32
    — rgb and the final counter of every sample —, dirs (n, samples_per_ray, 4) float32 — the unit direction drawn for it, then 0 —,
    basis (n, samples_per_ray, 9) float32 — vk_trace.h sh9 of that direction)"""
    lib = load()
    rp = DeviceScene.radiance_params(**params)
    probes = np.ascontiguousarray(probes, RAY_DTYPE).reshape(-1)
    n = len(probes)
    samples = np.zeros((n, rp.samples_per_ray, 4), np.float32)
    dirs = np.zeros((n, rp.samples_per_ray, 4), np.float32)
    basis = np.zeros((n, rp.samples_per_ray, 9), np.float32)
    st = lib.emu_probes(desc, C.byref(rp), probes.ctypes.data, n, samples.ctypes.data, dirs.ctypes.data, basis.ctypes.data, None)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_probes_last_error().decode()}")
    return samples, dirs, basis
