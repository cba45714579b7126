"""The frame's pixel sums recomputed exactly from a per-sample dump (vk_debug_render_samples).

Pixel sums are 64-bit fixed point (vk_kernels.h to_fixed_small / to_fixed, resolve_kernel), so the image is a pure integer function of the
per-sample radiances: whichever lane, wave, unit, launch or kernel instance traced a sample, the image must be this one, bit for bit."""
import numpy as np

ACCUM_SCALE = np.float32(2.0 ** 26)
ACCUM_SMALL = np.float32(31.999)
ACCUM_CLAMP = np.float32(1.0e10)
ACCUM_RANGE = np.float32(1.3e11)


def accum_clamp_for(spp):
    """vk_kernels.h accum_clamp_for: min(1e10, 1.3e11 / spp) in f32"""
    c = np.float32(ACCUM_RANGE / np.float32(spp))
    return c if c < ACCUM_CLAMP else ACCUM_CLAMP


def to_fixed(v, clampv):
    """the fixed-point value of each component of an (n, 3) float32 array of finite samples: x 2^26, truncated toward zero; a sample whose
    largest magnitude exceeds 31.999 is first clamped to +-clampv (the small path's int32 conversion and the 64-bit one agree below)"""
    v = np.asarray(v, np.float32)
    big = np.abs(v).max(axis=1, keepdims=True)
    w = np.where(big <= ACCUM_SMALL, v, np.clip(v, -clampv, clampv)).astype(np.float32)
    return np.trunc(w * ACCUM_SCALE).astype(np.int64)


def frame_sums(samples, width, height, spp, budget=None):
    """samples: the dump, (width * height * spp, 4) float32 with [pixel * spp + s] = (r, g, b, draw count bits).  Returns (sums
    (height, width, 3) int64, clamped samples): non-finite samples dropped (main.rs:192), the rest summed in fixed point.  budget: the
    spp the clamp is derived from (progressive rendering: the frame's total)"""
    s = np.asarray(samples, np.float32).reshape(height * width, spp, 4)[:, :, :3].reshape(-1, 3)
    keep = np.isfinite(s).all(axis=1)
    clampv = accum_clamp_for(budget or spp)
    fx = np.zeros((s.shape[0], 3), np.int64)
    fx[keep] = to_fixed(s[keep], clampv)
    big = np.abs(s[keep]).max(axis=1)
    clamped = int(((big > ACCUM_SMALL) & (big > clampv)).sum())
    sums = fx.reshape(height * width, spp, 3).sum(axis=1, dtype=np.int64)
    return sums.reshape(height, width, 3), clamped


def resolve(sums, spp):
    """resolve_kernel: float32(sum) * 2^-26 / float32(spp), each step in f32"""
    return ((np.asarray(sums, np.int64).astype(np.float32) * np.float32(1.0 / 2.0 ** 26)) / np.float32(spp)).astype(np.float32)


def exact_image(samples, width, height, spp):
    """(image (height, width, 3) float32, clamped samples) that the dump's samples must give"""
    sums, clamped = frame_sums(samples, width, height, spp)
    return resolve(sums, spp), clamped
