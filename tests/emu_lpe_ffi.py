"""ctypes binding of the light-path-layer emulator tests/emu/emu_lpe.cpp: the event code, the tag update, the rule match and the resolve of
a cell on the host, the kernels' own (vk_lpe.h through g++).  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_paths_ffi
from vecchio_amd import ffi

_bound = False
u32 = np.uint32


def load():
    global _bound
    lib = emu_paths_ffi.load()
    if not _bound:
        lib.emu_lpe_event_codes.restype = None
        lib.emu_lpe_event_codes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.emu_lpe_record.restype = None
        lib.emu_lpe_record.argtypes = [C.c_void_p] * 5 + [C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.emu_lpe_layers.restype = None
        lib.emu_lpe_layers.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p]
        lib.emu_lpe_resolve.restype = None
        lib.emu_lpe_resolve.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
        _bound = True
    return lib


def _u32(a):
    return np.ascontiguousarray(a, u32).reshape(-1)


def event_codes(status, lobe):
    status, lobe = _u32(status), _u32(lobe)
    out = np.full(len(status), 0x77, u32)
    load().emu_lpe_event_codes(status.ctypes.data, lobe.ctypes.data, len(status), out.ctypes.data)
    return out


def record(sig, term, bounce, ids, status, lobe, hit, material):
    """one bounce on the tables sig and term (uint32, contiguous; changed in place)"""
    assert sig.dtype == u32 and term.dtype == u32 and sig.flags.c_contiguous and term.flags.c_contiguous and len(sig) == len(term)
    ids, status, lobe, hit, material = (_u32(a) for a in (ids, status, lobe, hit, material))
    load().emu_lpe_record(status.ctypes.data, lobe.ctypes.data, hit.ctypes.data, material.ctypes.data, ids.ctypes.data, len(ids), len(sig),
                          bounce, sig.ctypes.data, term.ctypes.data)


def layers_of(rules, rest, status, depth, sig, term):
    arr = (ffi.LpeRule * max(1, len(rules)))(*rules)
    status, depth, sig, term = (_u32(a) for a in (status, depth, sig, term))
    out = np.full(len(status), 0x77, u32)
    load().emu_lpe_layers(C.cast(arr, C.c_void_p), len(rules), rest, status.ctypes.data, depth.ctypes.data, sig.ctypes.data, term.ctypes.data,
                          len(status), out.ctypes.data)
    return out


def resolve(cells, n):
    """cells (..., 4) int64 -> (rgb (..., 3), share (...)) float32"""
    cells = np.ascontiguousarray(cells, np.int64)
    shape = cells.shape[:-1]
    m = int(np.prod(shape, dtype=np.int64))
    rgb, share = np.full(shape + (3,), 7, np.float32), np.full(shape, 7, np.float32)
    load().emu_lpe_resolve(cells.ctypes.data, m, n, rgb.ctypes.data, share.ctypes.data)
    return rgb, share
