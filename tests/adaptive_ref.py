"""The adaptive judge (vk_progress_set_adaptive, vk_kernels.h adaptive_judge_kernel) restated in numpy: float64, the library's operation
order, so that every decision is reproduced exactly.  Inputs are what vk_debug_progress_moments returns (running fixed-point sums and
error moments, (height, width, 3), y up) and the tile map before the window was judged."""
import numpy as np

ACCUM_SCALE = 67108864.0          # 2^26 (vk_kernels.h ACCUM_SCALE)
TILE = 8


def tile_grid(width, height):
    return (width + TILE - 1) // TILE, (height + TILE - 1) // TILE


def partition_mask(width, height, rank=0, world=1):
    """(tiles_y, tiles_x) bool: the tiles of the partition rank of world (tile t = row-major index, tile row 0 at the bottom)"""
    tx, ty = tile_grid(width, height)
    return (np.arange(tx * ty) % world == rank).reshape(ty, tx)


def variance(run, m2, n, k):
    """the batch-means variance per component, vk_progress_stderr's operation order: mean = run / 2^26 / N,
    v = (m2 - N * mean * mean) / ((k - 1) * N); n and k broadcast against run (per pixel)"""
    N = np.asarray(n, np.float64)
    kk = np.asarray(k, np.float64)
    mean = run.astype(np.float64) / ACCUM_SCALE / N
    v = (m2 - N * mean * mean) / ((kk - 1.0) * N)
    return mean, v


def pixel_converged(run, m2, n, k, abs_tol, rel_tol):
    """(height, width) bool: every component has v <= (abs_tol + rel_tol * |mean|)^2 (tolerances as float32, widened to double)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        mean, v = variance(run, m2, n, k)
        tol = np.float64(np.float32(abs_tol)) + np.float64(np.float32(rel_tol)) * np.abs(mean)
        return (v <= tol * tol).all(axis=2)


def judge(run, m2, tile_n, done, steps, abs_tol, rel_tol, min_samples, min_steps, rank=0, world=1):
    """The tiles the window that brought the handle to (done, steps) freezes: (tiles_y, tiles_x) bool.  tile_n = the map BEFORE the
    judge (0 = active, as vk_progress_tile_samples' map minus the active tiles' samples_done); tiles outside the partition never are."""
    height, width = run.shape[:2]
    tx, ty = tile_grid(width, height)
    active = partition_mask(width, height, rank, world) & (np.asarray(tile_n) == 0)
    if done < min_samples or steps < min_steps:
        return np.zeros((ty, tx), bool)
    conv = np.ones((ty * TILE, tx * TILE), bool)              # pixels outside the image (edge tiles) do not vote
    conv[:height, :width] = pixel_converged(run, m2, done, steps, abs_tol, rel_tol)
    tile_ok = conv.reshape(ty, TILE, tx, TILE).all(axis=(1, 3))
    return active & tile_ok


def stderr(run, m2, tile_n, tile_k):
    """vk_progress_stderr of an adaptive handle: per pixel the tile's own N and k (maps (tiles_y, tiles_x)), float32 (height, width, 3)"""
    height, width = run.shape[:2]
    n = np.repeat(np.repeat(np.asarray(tile_n, np.float64), TILE, 0), TILE, 1)[:height, :width, None]
    k = np.repeat(np.repeat(np.asarray(tile_k, np.float64), TILE, 0), TILE, 1)[:height, :width, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        _, v = variance(run, m2, n, k)
    return np.sqrt(np.where(v > 0.0, v, 0.0)).astype(np.float32)


def tile_pixels(width, height):
    """(tiles_y, tiles_x): in-image pixels of every tile"""
    tx, ty = tile_grid(width, height)
    w = np.minimum(TILE, width - np.arange(tx) * TILE)
    h = np.minimum(TILE, height - np.arange(ty) * TILE)
    return h[:, None] * w[None, :]
