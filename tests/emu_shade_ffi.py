"""ctypes binding of the shade emulator tests/emu/emu_shade.cpp (vk_trace.h shade_hit on the host) and the loop of vk_shade_hits' contract
on the two emulators.  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_queries_ffi
from vecchio_amd import ffi
from vecchio_amd.scene import HIT_DTYPE, PATH_STATE_DTYPE, RAY_DTYPE, SHADED_DTYPE, DeviceScene, make_path_states, wavefront_loop

_bound = False


def load():
    global _bound
    lib = emu_queries_ffi.load()
    if not _bound:
        lib.emu_shade.restype = C.c_int
        lib.emu_shade.argtypes = [C.POINTER(ffi.SceneDesc), C.POINTER(ffi.ShadeParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                  C.c_void_p, C.POINTER(C.c_uint32)]
        lib.emu_shade_last_error.restype = C.c_char_p
        _bound = True
    return lib


def shade_hits(desc, rays, hits, states, **params):
    """what DeviceScene.shade_hits returns, computed on the host.  params: DeviceScene.shade_params()'s keywords."""
    lib = load()
    sp = DeviceScene.shade_params(**params)
    rays = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
    hits = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1)
    n = len(rays)
    assert len(hits) == n and len(states) == n
    out = np.zeros(n, SHADED_DTYPE)
    st = lib.emu_shade(desc, C.byref(sp), rays.ctypes.data, hits.ctypes.data, states.ctypes.data, n, out.ctypes.data, None)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_shade_last_error().decode()}")
    return out


def wavefront(desc, rays, seed=0, first_index=0, sample=0, **params):
    """what DeviceScene.wavefront_radiance returns with return_bounces, computed by the rays emulator and the shade emulator"""
    rays = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
    final, bounces = wavefront_loop(lambda r, s, fi: emu_queries_ffi.trace_rays(desc, r, s, fi)[0],
                                    lambda r, h, s: shade_hits(desc, r, h, s, **params), rays,
                                    make_path_states(len(rays), seed, first_index, sample), seed, first_index)
    res = np.zeros((len(rays), 4), np.float32)
    res[:, :3] = final["acc"]
    res[:, 3] = np.ascontiguousarray(final["counter"]).view(np.float32)
    return res, bounces
