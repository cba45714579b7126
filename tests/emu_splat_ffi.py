"""ctypes binding of the splat emulator tests/emu/emu_splat.cpp: vk_splat_deposit on the host, with the kernels' own footprint code
(vk_splat.h splat_weights through g++).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_paths_ffi
from vecchio_amd import ffi
from vecchio_amd.scene import PATH_STATE_DTYPE

_bound = False
COUNTERS = ("deposited", "dropped", "clamped", "skipped", "contributions")


def load():
    global _bound
    lib = emu_paths_ffi.load()
    if not _bound:
        lib.emu_splat_deposit.restype = C.c_int
        lib.emu_splat_deposit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.POINTER(ffi.SplatParams), C.c_void_p, C.POINTER(C.c_uint64 * 5)]
        lib.emu_splat_last_error.restype = C.c_char_p
        _bound = True
    return lib


def deposit(states, status, width, height, spp, sp, positions=None, sums=None):
    """tests/splat_ref.py deposit()'s twin in C++: (sums (height, width, 4) int64, dict of the five device counters)"""
    lib = load()
    states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1)
    status = np.ascontiguousarray(status, np.uint32).reshape(-1)
    sums = np.zeros((height, width, 4), np.int64) if sums is None else np.ascontiguousarray(sums, np.int64).copy()
    pos = None
    if positions is not None:
        positions = np.ascontiguousarray(positions, np.float32)
        assert positions.size == 2 * len(states)
        pos = positions.ctypes.data
    c = (C.c_uint64 * 5)()
    params = ffi.SplatParams(*sp)
    st = lib.emu_splat_deposit(states.ctypes.data, status.ctypes.data, len(states), pos, width, height, spp, C.byref(params),
                               sums.ctypes.data, C.byref(c))
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_splat_last_error().decode()}")
    return sums, dict(zip(COUNTERS, (int(v) for v in c)))
