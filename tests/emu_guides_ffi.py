"""ctypes binding of tests/emu/emu_guides.cpp (vk_trace.h guide_sample on the host).  TESTS ONLY."""
import ctypes as C
import os

import numpy as np

import emu_ffi
from vecchio_amd import ffi

CHANNELS = ("albedo", "normal", "depth", "coverage", "bounces")
_bound = False


def load():
    global _bound
    from vecchio_amd import build
    build.build_emu()                  # (a library built before emu_guides.cpp joined it is stale by its stamp)
    lib = emu_ffi.load()
    if not _bound:
        lib.emu_guides.restype = C.c_int
        lib.emu_guides.argtypes = [C.POINTER(ffi.SceneDesc), C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_float, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
        lib.emu_guides_last_error.restype = C.c_char_p
        _bound = True
    return lib


def _guides(desc, cam, p, first_sample, n, max_bounces, fuzz_max, mode, threads):
    lib = load()
    out = np.zeros((p.height, p.width) + ((n, 10) if mode == 0 else (9,)), np.float32)
    features = C.c_uint32()
    st = lib.emu_guides(desc, C.byref(cam), C.byref(p), first_sample, n, max_bounces, fuzz_max, mode, out.ctypes.data,
                        threads or (os.cpu_count() or 1), C.byref(features))
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_guides_last_error().decode()}")
    return out, features.value


def guide_samples(desc, cam, p, first_sample, n, max_bounces=4, fuzz_max=0.0, threads=None):
    """guide_sample of samples first_sample .. first_sample + n - 1 of every pixel: a list of n dicts in the form of a single-sample
    vk_render_guides call — albedo, normal (h, w, 3), depth (inf where coverage is 0), coverage, bounces (h, w); a dropped sample has
    zeros and coverage 0 — plus guide_sample's own verdict 'dropped' (h, w) bool; and the linearised scene's features"""
    out, features = _guides(desc, cam, p, first_sample, n, max_bounces, fuzz_max, 0, threads)
    res = []
    z = np.float32(0)
    for k in range(n):
        dropped = out[:, :, k, 8] != 0.0
        covered = (out[:, :, k, 7] != 0.0) & ~dropped
        res.append(dict(albedo=np.where(dropped[..., None], z, out[:, :, k, 0:3]).astype(np.float32),
                        normal=np.where(dropped[..., None], z, out[:, :, k, 3:6]).astype(np.float32),
                        depth=np.where(covered, out[:, :, k, 6], np.float32(np.inf)).astype(np.float32),
                        coverage=covered.astype(np.float32), bounces=np.where(dropped, z, out[:, :, k, 9]).astype(np.float32),
                        dropped=dropped))
    return res, features


def guide_window(desc, cam, p, first_sample, n, max_bounces=4, fuzz_max=0.0, threads=None):
    """the window [first_sample, first_sample + n) aggregated in specular_guides_kernel's order: what vk_render_guides returns"""
    out, _ = _guides(desc, cam, p, first_sample, n, max_bounces, fuzz_max, 1, threads)
    return dict(albedo=out[..., 0:3].copy(), normal=out[..., 3:6].copy(), depth=out[..., 6].copy(), coverage=out[..., 7].copy(),
                bounces=out[..., 8].copy())
