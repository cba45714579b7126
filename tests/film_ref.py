"""What tests/test_film_emu.py and tests/test_gpu_film.py share: a film's id <-> (pixel, sample) rule, the deposit restated in numpy on
top of tests/exact_sums.py, and the pixel patterns and radiance values the deposit is tried on."""
import numpy as np

import exact_sums as E
from vecchio_amd import ffi
from vecchio_amd.scene import PATH_STATE_DTYPE

f32 = np.float32
DEPOSITING = (ffi.VK_SHADE_MISS, ffi.VK_SHADE_ENDED, ffi.VK_PATHS_CULLED)


def ids_of(width, x0, y0, w, h, first_sample, n_samples):
    """(pixel, sample) of every id of a window of a width-wide frame: id = ((y - y0) * w + (x - x0)) * n_samples + k"""
    i = np.arange(w * h * n_samples)
    wp, k = i // n_samples, i % n_samples
    x, y = x0 + wp % w, y0 + wp // w
    return (y * width + x).astype(np.uint32), (first_sample + k).astype(np.uint32)


def dump_index(width, spp, x0, y0, w, h, first_sample, n_samples):
    """where each id's sample sits in vk_debug_render_samples' dump: [pixel * spp + s]"""
    pixel, s = ids_of(width, x0, y0, w, h, first_sample, n_samples)
    return pixel.astype(np.int64) * spp + s


def deposit(states, status, width, height, spp, sums=None):
    """vk_film_deposit in numpy: (sums (height, width, 3) int64 — added to where given —, dict of the four counters)"""
    states = np.ascontiguousarray(states, PATH_STATE_DTYPE).reshape(-1)
    status = np.ascontiguousarray(status, np.uint32).reshape(-1)
    n_pixels = width * height
    sums = np.zeros((height, width, 3), np.int64) if sums is None else sums.copy()
    flat = sums.reshape(n_pixels, 3)
    ours = np.isin(status, DEPOSITING) & (states["pixel"] < n_pixels)
    acc = states["acc"].astype(f32)
    finite = np.isfinite(acc).all(axis=1)
    dep = ours & finite
    clampv = E.accum_clamp_for(spp)
    big = np.abs(acc[dep]).max(axis=1) if dep.any() else np.zeros(0, f32)
    np.add.at(flat, states["pixel"][dep].astype(np.int64), E.to_fixed(acc[dep], clampv) if dep.any() else np.zeros((0, 3), np.int64))
    counters = dict(deposited=int(dep.sum()), dropped=int((ours & ~finite).sum()),
                    clamped=int(((big > E.ACCUM_SMALL) & (big > clampv)).sum()), skipped=int((~ours).sum()))
    return sums, counters


def counters_of(info):
    return {k: int(getattr(info, k)) for k in ("deposited", "dropped", "clamped", "skipped")}


def pixel_patterns(n, n_pixels):
    """name -> pixel of each of n results: all equal; alternating A, B; runs of 3 (they straddle the wave boundaries: 64 is no multiple
    of 3); a run of 100 inside distinct pixels; distinct pixels with every seventh outside the frame"""
    i = np.arange(n)
    out = {"equal": np.full(n, 5 % n_pixels), "alternating": np.where(i % 2 == 0, 3 % n_pixels, 11 % n_pixels), "runs3": (i // 3) % n_pixels,
           "run100": np.where((i >= 20) & (i < 120), 7 % n_pixels, (i + 13) % n_pixels),
           "outside": np.where(i % 7 == 3, n_pixels + i, i % n_pixels)}
    return {k: v.astype(np.uint32) for k, v in out.items()}


def radiances(n, spp, seed=0):
    """(n, 3) float32: ordinary values, with the deposit's special cases sprinkled over them at fixed strides — NaN, +-inf, 31.999 and the
    float above it, beyond the clamp in both signs, below 2^-26, negative"""
    rng = np.random.default_rng(seed + n)
    acc = (rng.random((n, 3)) * 2.0).astype(f32)
    clampv = E.accum_clamp_for(spp)
    special = [(np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -np.inf), (31.999, 1.0, -31.999), (np.nextafter(f32(31.999), f32(40)), 1.0, 2.0),
               (clampv * f32(2), 1.0, 1.0), (1.0, -clampv * f32(3), 40.0), (2.0 ** -27, -2.0 ** -27, 2.0 ** -26), (-0.75, -1e-3, 1e3),
               (clampv, 0.0, 0.0)]
    for j, v in enumerate(special):
        acc[j::len(special) + 3][::2] = np.array(v, f32)
    return acc


def states_for(pixel, acc, seed=0):
    st = np.zeros(len(pixel), PATH_STATE_DTYPE)
    st["thr"], st["depth"], st["acc"], st["seed"], st["pixel"], st["sample"] = 1.0, 1, acc, seed, pixel, 0
    return st
