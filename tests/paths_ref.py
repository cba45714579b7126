"""What tests/test_paths_emu.py and tests/test_gpu_paths.py share: the compaction of a path batch's bounce restated in numpy (boolean
indexing plus a scatter by id), the status patterns and sizes it is tried on, and the kernel constants the sizes are chosen around."""
import numpy as np

from vecchio_amd import ffi
from vecchio_amd.scene import PATH_STATE_DTYPE, RAY_DTYPE, SHADED_DTYPE

# vk_kernels.h: items per workgroup of the count and move passes, workgroup counts per pass of the scan (tests/test_paths_abi.py holds
# these two to the kernel constants)
PATHS_T = 256
PATHS_SCAN_T = 256
# one workgroup more than a single pass of the scan covers, and a ragged last workgroup: 65536 + 256 + 5 items (below 2^20)
N_SCAN_TWO_PASSES = PATHS_T * PATHS_SCAN_T + PATHS_T + 5
SIZES = sorted({1, 63, 64, 65, 255, 256, 257, PATHS_T - 1, PATHS_T, PATHS_T + 1, 3 * PATHS_T + 5, N_SCAN_TWO_PASSES})
CANARY = 0xA5
RETIRING = (ffi.VK_SHADE_MISS, ffi.VK_SHADE_ENDED, ffi.VK_SHADE_BAD_HIT, ffi.VK_PATHS_CULLED)


def compact(items, ids, n_ids, canary=CANARY):
    """what DeviceScene.debug_compact_paths returns: (rays, states, ids_out, result_state, result_status, counts)"""
    items = np.ascontiguousarray(items, SHADED_DTYPE).reshape(-1)
    ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
    n = len(items)
    assert len(ids) == n and (n == 0 or int(ids.max()) < n_ids)
    outs = [np.zeros(n, RAY_DTYPE), np.zeros(n, PATH_STATE_DTYPE), np.zeros(n, np.uint32), np.zeros(n_ids, PATH_STATE_DTYPE),
            np.zeros(n_ids, np.uint32)]
    for a in outs:
        a.view(np.uint8)[:] = canary
    rays, states, ids_out, result_state, result_status = outs
    go = items["status"] == ffi.VK_SHADE_SCATTERED
    m = int(go.sum())
    rays[:m] = items["next"][go]
    states[:m] = items["state"][go]
    ids_out[:m] = ids[go]
    result_state[ids[~go]] = items["state"][~go]
    result_status[ids[~go]] = items["status"][~go]
    counts = np.bincount(np.minimum(items["status"], 4), minlength=5).astype(np.uint64)
    return rays, states, ids_out, result_state, result_status, counts


def patterns(n):
    """name -> status array of n items: all scattered; none; only the first; only the last; alternating; runs of 64 and of 65; random
    with survivor shares 0.5 and 0.01, the four retiring statuses mixed in"""
    S, E = ffi.VK_SHADE_SCATTERED, ffi.VK_SHADE_ENDED
    i = np.arange(n)
    out = {"all": np.full(n, S), "none": np.full(n, E), "first": np.where(i == 0, S, E), "last": np.where(i == n - 1, S, E),
           "alternating": np.where(i % 2 == 0, S, E), "runs64": np.where((i // 64) % 2 == 0, S, E), "runs65": np.where((i // 65) % 2 == 1, S, E)}
    for share in (0.5, 0.01):
        rng = np.random.default_rng(1000 + n + int(share * 100))
        out[f"random{share}"] = np.where(rng.random(n) < share, S, rng.choice(RETIRING, n))
    return {k: v.astype(np.uint32) for k, v in out.items()}


def items_for(status, seed=0):
    """(items, ids, n_ids): SHADED_DTYPE records with the given statuses and recognisable, distinct bytes everywhere else; ids ascending
    but not contiguous (every third number from 2)"""
    n = len(status)
    rng = np.random.default_rng(seed + n)
    items = np.zeros(n, SHADED_DTYPE)
    items.view(np.uint32).reshape(n, 24)[:] = rng.integers(0, 2 ** 32, (n, 24), dtype=np.uint64).astype(np.uint32)
    items["status"] = status
    ids = (2 + 3 * np.arange(n)).astype(np.uint32)
    return items, ids, 3 * n + 2


def assert_same(got, want, what=""):
    names = ("rays", "states", "ids_out", "result_state", "result_status", "counts")
    for name, g, w in zip(names, got, want):
        gb, wb = np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)
        assert gb.shape == wb.shape, (what, name, gb.shape, wb.shape)
        if not np.array_equal(gb, wb):
            k = int(np.flatnonzero(gb != wb)[0]) // g.dtype.itemsize
            raise AssertionError(f"{what}: {name} differs first at entry {k}: got {g[k]}, want {w[k]}")
