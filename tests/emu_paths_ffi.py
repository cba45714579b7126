"""ctypes binding of the path-batch emulator tests/emu/emu_paths.cpp (vk_trace.h trace_path on the host) and a path batch's loop on the
emulators: the path-stream trace, the shade emulator, the numpy compaction of tests/paths_ref.py.  TESTS ONLY."""
import ctypes as C

import numpy as np

import emu_queries_ffi
import emu_shade_ffi
import paths_ref
from vecchio_amd import ffi
from vecchio_amd.scene import HIT_DTYPE, PATH_STATE_DTYPE, RAY_DTYPE, SHADED_DTYPE, make_path_states

_bound = False


def load():
    global _bound
    lib = emu_queries_ffi.load()
    emu_shade_ffi.load()
    if not _bound:
        lib.emu_paths_trace.restype = C.c_int
        lib.emu_paths_trace.argtypes = [C.POINTER(ffi.SceneDesc), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32)]
        lib.emu_paths_trace_last_error.restype = C.c_char_p
        _bound = True
    return lib


def trace_paths(desc, rays, states):
    """a path batch's trace step: (HIT_DTYPE array, the states with their counters advanced by what a medium drew)"""
    lib = load()
    rays = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
    states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1).copy()
    n = len(rays)
    assert len(states) == n
    hits = np.zeros(n, HIT_DTYPE)
    st = lib.emu_paths_trace(desc, rays.ctypes.data, states.ctypes.data, n, hits.ctypes.data, None)
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib.emu_paths_trace_last_error().decode()}")
    return hits, states


class Batch:
    """vecchio_amd.scene.PathBatch on the emulators: begin / step (one bounce) / read / cull / results with the same meaning"""

    def __init__(self, desc, **params):
        self.desc, self.params = desc, params

    def begin(self, rays, states):
        self.rays = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1).copy()
        self.states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1).copy()
        n = len(self.rays)
        self.ids = np.arange(n, dtype=np.uint32)
        self.result_state, self.result_status = np.zeros(n, PATH_STATE_DTYPE), np.zeros(n, np.uint32)
        self.retired = np.zeros(5, np.uint64)

    @property
    def live(self):
        return len(self.ids)

    def _compact(self, items):
        n_ids = len(self.result_state)
        rays, states, ids, rs, rst, counts = paths_ref.compact(items, self.ids, n_ids)
        m = int(counts[ffi.VK_SHADE_SCATTERED])
        gone = self.ids[items["status"] != ffi.VK_SHADE_SCATTERED]
        self.result_state[gone], self.result_status[gone] = rs[gone], rst[gone]
        self.rays, self.states, self.ids = rays[:m].copy(), states[:m].copy(), ids[:m].copy()
        counts[ffi.VK_SHADE_SCATTERED] = 0
        self.retired += counts

    def step(self):
        hits, advanced = trace_paths(self.desc, self.rays, self.states)
        out = emu_shade_ffi.shade_hits(self.desc, self.rays, hits, advanced, **self.params)
        self._compact(out)
        return hits, out

    def read(self):
        return self.ids.copy(), self.rays.copy(), self.states.copy()

    def cull(self, keep, scale=None):
        keep = np.asarray(keep, np.uint8) != 0
        items = np.zeros(self.live, SHADED_DTYPE)
        items["next"], items["state"] = self.rays, self.states
        if scale is not None:
            thr = items["state"]["thr"]
            thr[keep] = (thr[keep] * np.asarray(scale, np.float32)[keep, None]).astype(np.float32)
        items["status"] = np.where(keep, ffi.VK_SHADE_SCATTERED, ffi.VK_PATHS_CULLED)
        items["lobe"] = 0xFFFFFFFF
        self._compact(items)

    def results(self):
        states, status = self.result_state.copy(), self.result_status.copy()
        states[self.ids], status[self.ids] = self.states, ffi.VK_PATHS_LIVE
        return states, status


def run(desc, rays, seed=0, first_index=0, sample=0, **params):
    """a batch begun with the contract's states and stepped to its end: ((n, 4) float32 — acc and the counter's bit pattern —, the list
    of every bounce's (ids, rays, states) after its compaction)"""
    rays = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
    b = Batch(desc, **params)
    b.begin(rays, make_path_states(len(rays), seed, first_index, sample))
    bounces = []
    while b.live:
        b.step()
        bounces.append(b.read())
    states, _ = b.results()
    res = np.zeros((len(rays), 4), np.float32)
    res[:, :3] = states["acc"]
    res[:, 3] = np.ascontiguousarray(states["counter"]).view(np.float32)
    return res, bounces
