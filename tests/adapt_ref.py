"""A film's tile runs and error moments (vk_adapt_*) in numpy, shared by tests/test_adapt_emu.py and tests/test_gpu_adapt.py: the
sequence of a tile run for a tile map as include/vecchio_amd.h writes it down, and the fold of a close (accumulate_resolve_kernel's
expression in float64, in its order).  The judge and the standard error are tests/adaptive_ref.py's."""
import numpy as np

from adaptive_ref import ACCUM_SCALE, TILE, judge, stderr, tile_grid, tile_pixels      # noqa: F401  (re-exported)


def sequence(width, height, tile_n, n_samples, samples_done=0):
    """(pixel, sample) uint32 arrays, one entry per path q of a tile run of n_samples over the active tiles of tile_n ((tiles_y, tiles_x),
    0 = active): active tiles in ascending tile index, a tile's in-image pixels row by row from its bottom-left, n_samples paths a pixel;
    pixel = y * width + x, sample = samples_done + k"""
    tx_n, ty_n = tile_grid(width, height)
    tile_n = np.asarray(tile_n).reshape(ty_n, tx_n)
    pixel = []
    for t in range(tx_n * ty_n):
        ty, tx = divmod(t, tx_n)
        if tile_n[ty, tx] != 0:
            continue
        tw, th = min(TILE, width - TILE * tx), min(TILE, height - TILE * ty)
        for j in range(tw * th):
            pixel.append((TILE * ty + j // tw) * width + TILE * tx + j % tw)
    pixel = np.repeat(np.asarray(pixel, np.uint32), n_samples)
    sample = np.tile(np.arange(n_samples, dtype=np.uint32), len(pixel) // n_samples) + np.uint32(samples_done)
    return pixel, sample.astype(np.uint32)


def active_mask(width, height, tile_n):
    """(height, width) bool: the pixels of the active tiles"""
    tx_n, ty_n = tile_grid(width, height)
    act = np.asarray(tile_n).reshape(ty_n, tx_n) == 0
    return np.repeat(np.repeat(act, TILE, 0), TILE, 1)[:height, :width]


def fold(sums, prev, m2, tile_n, n_samples):
    """a close's fold for the pixels of the active tiles: w = sums - prev, prev = sums, s = w * 2^-26, m2 += s * s / n_samples.  sums and
    prev int64 (height, width, 3), m2 float64; returns the new (prev, m2)"""
    height, width = sums.shape[:2]
    act = active_mask(width, height, tile_n)[:, :, None]
    w = sums - prev
    s = w.astype(np.float64) * (1.0 / ACCUM_SCALE)
    return np.where(act, sums, prev), np.where(act, m2 + s * s / np.float64(n_samples), m2)


def resolve(prev, tile_n, samples_done):
    """vk_adapt_resolve: float32 (height, width, 3), every pixel over its tile's own count"""
    height, width = prev.shape[:2]
    tx_n, ty_n = tile_grid(width, height)
    n = np.asarray(tile_n).reshape(ty_n, tx_n)
    n = np.where(n == 0, samples_done, n)
    n = np.repeat(np.repeat(n, TILE, 0), TILE, 1)[:height, :width, None].astype(np.float32)
    return (prev.astype(np.float32) * np.float32(1.0 / ACCUM_SCALE)) / n


def tile_maps(width, height):
    """the tile maps the tests impose, by name: 0 = active, 8 = frozen with 8 samples"""
    tx_n, ty_n = tile_grid(width, height)
    t = np.arange(tx_n * ty_n).reshape(ty_n, tx_n)
    frozen = np.uint32(8)
    top_right = np.full((ty_n, tx_n), frozen, np.uint32)
    top_right[-1, -1] = 0
    return {
        "all active": np.zeros((ty_n, tx_n), np.uint32),
        "checkerboard": np.where((t // tx_n + t % tx_n) % 2 == 0, 0, frozen).astype(np.uint32),
        "top-right only": top_right,
        "tile 0 frozen": np.where(t == 0, frozen, 0).astype(np.uint32),
        "none active": np.full((ty_n, tx_n), frozen, np.uint32),
    }
