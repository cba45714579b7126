"""ctypes binding of the upsampling emulator tests/emu/emu_upsample.cpp: the prepare pass and the filter on the host, the kernels' own
per-pixel code (vk_upsample.h through g++), and the library's ratios and AUTO rule.  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_paths_ffi

_bound = False


def load():
    global _bound
    lib = emu_paths_ffi.load()
    if not _bound:
        lib.emu_upsample_apply.restype = C.c_int
        lib.emu_upsample_apply.argtypes = [C.c_void_p] * 5 + [C.c_uint32] * 4 + [C.c_void_p] * 3 + [C.c_float, C.c_uint32, C.c_float] + \
            [C.c_void_p] * 3
        lib.emu_upsample_auto_form.restype = C.c_uint32
        lib.emu_upsample_auto_form.argtypes = [C.c_uint32] * 4
        lib.emu_upsample_ratios.restype = C.c_int
        lib.emu_upsample_ratios.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        lib.emu_upsample_last_error.restype = C.c_char_p
        _bound = True
    return lib


def _arr(a, n):
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, np.float32)
    assert a.size == n
    return a, a.ctypes.data


def apply(color, W, H, stderr3=None, albedo=None, normal=None, depth=None, albedo_hi=None, normal_hi=None, depth_hi=None,
          sigma_z=1.0, normal_squarings=7, albedo_floor=1e-3, want_stderr=True):
    """tests/upsample_ref.py apply()'s twin in C++: the same arguments, the same four results"""
    lib = load()
    color = np.ascontiguousarray(color, np.float32)
    h, w = color.shape[:2]
    lo = [_arr(a, w * h * c) for a, c in ((color, 3), (stderr3, 3), (albedo, 3), (normal, 3), (depth, 1))]
    hi = [_arr(a, W * H * c) for a, c in ((albedo_hi, 3), (normal_hi, 3), (depth_hi, 1))]
    out = np.full((H, W, 3), 7.0, np.float32)
    se = np.full((H, W, 3), 7.0, np.float32) if want_stderr else None
    counts = np.full(2, 7, np.uint64)
    st = lib.emu_upsample_apply(*[k[1] for k in lo], w, h, W, H, *[k[1] for k in hi], float(np.float32(sigma_z)), normal_squarings,
                                float(np.float32(albedo_floor)), out.ctypes.data, se.ctypes.data if want_stderr else None, counts.ctypes.data)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_upsample_last_error().decode()}")
    return out, se, int(counts[0]), int(counts[1])


def auto_form(w, h, W, H):
    return int(load().emu_upsample_auto_form(w, h, W, H))


def ratios(lo, hi):
    r = np.zeros(2, np.float32)
    assert load().emu_upsample_ratios(lo, hi, r.ctypes.data) == 0
    return r[0], r[1]
