"""ctypes binding of the glare emulator tests/emu/emu_glare.cpp: every level of the pyramid and the composite on the host, the kernels' own
per-pixel code (vk_glare.h through g++), and the library's weights and launch plan.  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_paths_ffi

_bound = False


def load():
    global _bound
    lib = emu_paths_ffi.load()
    if not _bound:
        lib.emu_glare_apply.restype = C.c_int
        lib.emu_glare_apply.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p]
        lib.emu_glare_weights.restype = C.c_int
        lib.emu_glare_weights.argtypes = [C.c_uint32, C.c_float, C.c_void_p]
        lib.emu_glare_tail_level.restype = C.c_uint32
        lib.emu_glare_tail_level.argtypes = [C.c_uint32, C.c_uint32]
        lib.emu_glare_launch_count.restype = C.c_uint32
        lib.emu_glare_launch_count.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.emu_glare_last_error.restype = C.c_char_p
        _bound = True
    return lib


def apply(I, levels=6, strength=0.15, falloff=1.0, threshold=0.0):
    """tests/glare_ref.py apply()'s twin in C++: an (H, W, 3) float32 frame, y up -> the same shape"""
    lib = load()
    I = np.ascontiguousarray(I, np.float32)
    H, W = I.shape[:2]
    out = np.full((H, W, 3), 7.0, np.float32)
    st = lib.emu_glare_apply(I.ctypes.data, W, H, levels, float(np.float32(strength)), float(np.float32(falloff)),
                             float(np.float32(threshold)), out.ctypes.data)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_glare_last_error().decode()}")
    return out


def weights(levels, falloff):
    lib = load()
    c = np.zeros(levels, np.float32)
    assert lib.emu_glare_weights(levels, float(np.float32(falloff)), c.ctypes.data) == 0
    return c


def tail_level(W, H):
    return int(load().emu_glare_tail_level(W, H))


def launch_count(W, H, levels, form):
    return int(load().emu_glare_launch_count(W, H, levels, form))
