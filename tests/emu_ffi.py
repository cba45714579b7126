"""ctypes binding of tests/emu (host build of the kernel's per-lane logic).  TESTS ONLY."""
import ctypes as C
import os

import numpy as np

from vecchio_amd import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libemu.so")
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(EMU_SO):
        from vecchio_amd import build
        build.build_emu()
    lib = C.CDLL(EMU_SO)
    lib.emu_render.restype = C.c_int
    lib.emu_render.argtypes = [C.POINTER(ffi.SceneDesc), C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_void_p, C.c_void_p,
                               C.c_int, C.POINTER(C.c_uint64), C.c_void_p]
    lib.emu_aov.restype = C.c_int
    lib.emu_aov.argtypes = [C.POINTER(ffi.SceneDesc), C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_uint32, C.c_uint32, C.c_int,
                            C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
    lib.emu_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def render_samples(desc, cam, p, threads=None):
    """returns (image, per_sample[n,4], steps, info) — per_sample[:,3] is the draw count bit pattern"""
    lib = load()
    img = np.zeros((p.height, p.width, 3), np.float32)
    ps = np.zeros((p.width * p.height * p.samples_per_pixel, 4), np.float32)
    steps = C.c_uint64()
    info = (C.c_uint32 * 4)()
    st = lib.emu_render(desc, C.byref(cam), C.byref(p), img.ctypes.data, ps.ctypes.data, threads or (os.cpu_count() or 1), C.byref(steps), info)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_last_error().decode()}")
    return img, ps, steps.value, list(info)


def take_redo_stats():
    """exact re-treeing: (samples rendered again on the tree as handed over, segments walked) since the last call"""
    lib = load()
    out = (C.c_uint64 * 2)()
    lib.emu_take_redo_stats(out)
    return int(out[0]), int(out[1])


def take_visit_counts():
    """(box tests, sphere tests) of every walk since the last call — second walks and samples rendered again included; sphere tests are
    counted for scenes of spheres only (other scenes: primitive steps)"""
    lib = load()
    out = (C.c_uint64 * 2)()
    lib.emu_take_visit_counts(out)
    return int(out[0]), int(out[1])


def _aov(desc, cam, p, first_sample, n, mode, width, threads):
    lib = load()
    out = np.zeros((p.height, p.width) + ((n, 9) if mode == 0 else (8,)), np.float32)
    features = C.c_uint32()
    st = lib.emu_aov(desc, C.byref(cam), C.byref(p), first_sample, n, mode, out.ctypes.data, threads or (os.cpu_count() or 1),
                     C.byref(features))
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_last_error().decode()}")
    return out, features.value


def aov_samples(desc, cam, p, first_sample, n, threads=None):
    """vk_trace.h aov_sample of samples first_sample .. first_sample + n - 1 of every pixel, on the tree as handed over: a list of n
    dicts in the form of a single-sample vk_render_aov call — albedo, normal (h, w, 3), depth (inf where coverage is 0), coverage (h, w);
    a dropped sample has zeros and coverage 0 — plus aov_sample's own verdict 'dropped' (h, w) bool; and the linearised scene's
    features (0: the sphere-only kernel instance, as vk_api.hip enqueue_aov picks)"""
    out, features = _aov(desc, cam, p, first_sample, n, 0, 9, threads)
    res = []
    for k in range(n):
        dropped = out[:, :, k, 8] != 0.0
        covered = (out[:, :, k, 7] != 0.0) & ~dropped
        res.append(dict(albedo=np.where(dropped[..., None], np.float32(0), out[:, :, k, 0:3]).astype(np.float32),
                        normal=np.where(dropped[..., None], np.float32(0), out[:, :, k, 3:6]).astype(np.float32),
                        depth=np.where(covered, out[:, :, k, 6], np.float32(np.inf)).astype(np.float32),
                        coverage=covered.astype(np.float32), dropped=dropped))
    return res, features


def aov_window(desc, cam, p, first_sample, n, threads=None):
    """the window [first_sample, first_sample + n) aggregated in aov_kernel's order (vk_kernels.h): what vk_render_aov returns"""
    out, _ = _aov(desc, cam, p, first_sample, n, 1, 8, threads)
    return dict(albedo=out[..., 0:3].copy(), normal=out[..., 3:6].copy(), depth=out[..., 6].copy(), coverage=out[..., 7].copy())
