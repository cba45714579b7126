"""ctypes binding of the film emulator tests/emu/emu_film.cpp: vk_film_emit's camera paths (vk_trace.h start_sample_core on the host) and
vk_film_deposit's sums in plain C++.  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_paths_ffi
from vecchio_amd import ffi
from vecchio_amd.scene import PATH_STATE_DTYPE, RAY_DTYPE

_bound = False


def load():
    global _bound
    lib = emu_paths_ffi.load()
    if not _bound:
        lib.emu_film_emit.restype = C.c_int
        lib.emu_film_emit.argtypes = [C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.POINTER(ffi.FilmWindow), C.c_void_p, C.c_void_p]
        lib.emu_film_deposit.restype = C.c_int
        lib.emu_film_deposit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64 * 4)]
        lib.emu_film_last_error.restype = C.c_char_p
        _bound = True
    return lib


def emit(cam, p, x0, y0, w, h, first_sample, n_samples):
    """(rays, states) of the window's camera paths, in id order"""
    lib = load()
    n = w * h * n_samples
    rays, states = np.zeros(n, RAY_DTYPE), np.zeros(n, PATH_STATE_DTYPE)
    win = ffi.FilmWindow(x0, y0, w, h, first_sample, n_samples)
    st = lib.emu_film_emit(C.byref(cam), C.byref(p), C.byref(win), rays.ctypes.data, states.ctypes.data)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_film_last_error().decode()}")
    return rays, states


def deposit(states, status, width, height, spp, sums=None):
    """tests/film_ref.py deposit()'s twin in C++: (sums (height, width, 3) int64, dict of the four counters)"""
    lib = load()
    states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1)
    status = np.ascontiguousarray(status, np.uint32).reshape(-1)
    sums = np.zeros((height, width, 3), np.int64) if sums is None else np.ascontiguousarray(sums, np.int64).copy()
    c = (C.c_uint64 * 4)()
    st = lib.emu_film_deposit(states.ctypes.data, status.ctypes.data, len(states), width * height, spp, sums.ctypes.data, C.byref(c))
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_film_last_error().decode()}")
    return sums, dict(zip(("deposited", "dropped", "clamped", "skipped"), (int(v) for v in c)))


def run(desc, cam, p, integrator, max_depth, window=None):
    """a window (default: the whole frame, every sample) emitted and stepped to its end on the emulators: (states, status) per id"""
    import shade_ref as S
    win = window or (0, 0, p.width, p.height, 0, p.samples_per_pixel)
    rays, states = emit(cam, p, *win)
    b = emu_paths_ffi.Batch(desc, **S.shade_kwargs(p, integrator, max_depth))
    b.begin(rays, states)
    while b.live:
        b.step()
    return b.results()
