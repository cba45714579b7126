"""ctypes binding of the display-transform emulator tests/emu/emu_tone.cpp: the histogram's classification, the curves and the transfers
on the host, the kernels' own (vk_tone.h through g++).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_paths_ffi

_bound = False


def load():
    global _bound
    lib = emu_paths_ffi.load()
    if not _bound:
        lib.emu_tone_histogram.restype = C.c_int
        lib.emu_tone_histogram.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.emu_tone_hable.restype = C.c_float
        lib.emu_tone_hable.argtypes = [C.c_float]
        lib.emu_tone_encode.restype = C.c_int
        lib.emu_tone_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_uint64,
                                        C.c_void_p]
        lib.emu_tone_last_error.restype = C.c_char_p
        _bound = True
    return lib


def histogram(rgb):
    """tests/tone_ref.py histogram()'s twin in C++: (bins (640,) uint32, counters (4,) uint64)"""
    rgb = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
    bins, counters = np.zeros(640, np.uint32), np.zeros(4, np.uint64)
    assert load().emu_tone_histogram(rgb.ctypes.data, len(rgb), bins.ctypes.data, counters.ctypes.data) == 0
    return bins, counters


def hable(v):
    return np.float32(load().emu_tone_hable(float(np.float32(v))))


def encode(rgb, curve, table, dither, E, p, seed=0):
    """tests/tone_ref.py encode()'s twin in C++: rgb (H, W, 3) float32, y up -> (H, W, 3) uint8, row 0 the top"""
    lib = load()
    rgb = np.ascontiguousarray(rgb, np.float32)
    H, W = rgb.shape[:2]
    out = np.full((H, W, 3), 0x77, np.uint8)
    tab = None if table is None else np.ascontiguousarray(table, np.float32)
    st = lib.emu_tone_encode(rgb.ctypes.data, W, H, curve, None if tab is None else tab.ctypes.data, int(bool(dither)), float(np.float32(E)),
                             float(np.float32(p)), int(seed), out.ctypes.data)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_tone_last_error().decode()}")
    return out
