"""A film's tile runs on the CPU (vk_adapt_begin's sequence; tests/emu/emu_adapt.cpp builds the top-up kernel's own index code,
vk_adapt.h adapt_locate).  On frames of whole and partial tiles and on tile maps from all active to none: the index function against the
numpy enumeration of tests/adapt_ref.py for every path, every (pixel, sample) of the active tiles exactly once, the emitted rays and
states against tests/emu_film_ffi.py's for the same (pixel, sample) byte for byte; and the moments of a tile run deposited in
tests/regen_ref.py's schedule order and folded by the reference, which no capacity moves.  tests/test_gpu_adapt.py holds the device
against the same references."""
import numpy as np
import pytest

import adapt_ref as A
import film_ref as F
import regen_ref as G
import shade_ref as S
from vecchio_amd import ffi

FRAMES = [(24, 16), (21, 13), (8, 8)]
MAPS = ["all active", "checkerboard", "top-right only", "tile 0 frozen", "none active"]
DONE = 2                      # the samples behind the run: the run's first sample


@pytest.fixture(scope="module")
def emu_adapt(built):
    import emu_adapt_ffi
    emu_adapt_ffi.load()
    return emu_adapt_ffi


def frame(host_scenes, width, height, spp=8, max_depth=None):
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    q = ffi.RenderParams.from_buffer_copy(p)
    q.width, q.height, q.samples_per_pixel = width, height, spp
    if max_depth is not None:
        q.max_depth = max_depth
    return desc, cam, q


@pytest.mark.parametrize("n_samples", [1, 3])
@pytest.mark.parametrize("which", MAPS)
@pytest.mark.parametrize("width,height", FRAMES)
def test_sequence_and_emitted_paths(width, height, which, n_samples, emu_adapt, host_scenes):
    import emu_film_ffi
    tile_n = A.tile_maps(width, height)[which]
    pixel, sample = A.sequence(width, height, tile_n, n_samples, DONE)
    total = len(pixel)
    act = A.active_mask(width, height, tile_n)
    assert total == int(act.sum()) * n_samples == emu_adapt.total(width, height, tile_n, n_samples)
    assert (total == 0) == (not (tile_n == 0).any())         # (the 8 x 8 frame is one tile: with tile 0 frozen nothing is active)
    # the index function, for every q; and from a start in the middle of a tile
    got_p, got_s = emu_adapt.sequence(width, height, tile_n, n_samples, DONE)
    assert np.array_equal(got_p, pixel) and np.array_equal(got_s, sample)
    if total > 5:
        first = total // 2 + 1
        got_p, got_s = emu_adapt.sequence(width, height, tile_n, n_samples, DONE, first, total - first - 1)
        assert np.array_equal(got_p, pixel[first:-1]) and np.array_equal(got_s, sample[first:-1])
    # every (pixel, sample) of the active tiles exactly once, nothing of a frozen tile
    seen = np.zeros((height * width, n_samples), int)
    np.add.at(seen, (pixel.astype(int), sample.astype(int) - DONE), 1)
    assert np.array_equal(seen, np.repeat(act.reshape(-1, 1), n_samples, 1).astype(int))
    # the rays and states: vk_film_emit's for the same (pixel, sample), byte for byte
    _, cam, q = frame(host_scenes, width, height)
    rays, states, ids = emu_adapt.emit(cam, q, tile_n, n_samples, DONE)
    assert np.array_equal(ids, np.arange(total, dtype=np.uint32))
    want_r, want_s = emu_film_ffi.emit(cam, q, 0, 0, width, height, DONE, n_samples)
    at = pixel.astype(np.int64) * n_samples + (sample.astype(np.int64) - DONE)
    assert rays.tobytes() == want_r[at].tobytes() and states.tobytes() == want_s[at].tobytes()
    if total:
        assert np.array_equal(states["pixel"], pixel) and np.array_equal(states["sample"], sample)


@pytest.fixture(scope="module")
def stepped(emu_adapt, host_scenes):
    """a tile run of the 21 x 13 frame on the checkerboard stepped whole on the emulators: lifetimes, final states, statuses"""
    import emu_paths_ffi
    width, height, n = 21, 13, 3
    desc, cam, q = frame(host_scenes, width, height, max_depth=12)
    tile_n = A.tile_maps(width, height)["checkerboard"]
    rays, states, _ = emu_adapt.emit(cam, q, tile_n, n, DONE)
    b = emu_paths_ffi.Batch(desc, **S.shade_kwargs(q, q.integrator, q.max_depth))
    b.begin(rays, states)
    hist = [b.read()[0]]
    while b.live:
        b.step()
        hist.append(b.read()[0])
    states, status = b.results()
    return q, tile_n, n, G.lifetimes_of(hist, len(rays)), states, status


@pytest.fixture(scope="module")
def whole_fold(stepped):
    """the moments of the run deposited at once: the reference every capacity must give"""
    q, tile_n, n, _, states, status = stepped
    sums, _ = F.deposit(states, status, q.width, q.height, q.samples_per_pixel)
    zero = np.zeros_like(sums)
    return sums, A.fold(sums, zero, np.zeros(sums.shape, np.float64), tile_n, n)


@pytest.mark.parametrize("capacity", [1, 64, 65, "total", "total + 7"])
def test_moments_do_not_depend_on_the_capacity(capacity, stepped, whole_fold):
    q, tile_n, n, life, states, status = stepped
    total = len(life)
    assert total == int(A.active_mask(q.width, q.height, tile_n).sum()) * n and life.max() > 3
    capacity = {"total": total, "total + 7": total + 7}.get(capacity, capacity)
    sums = None
    for b in G.schedule(life, capacity):
        sums, _ = F.deposit(states[b["retired"]], status[b["retired"]], q.width, q.height, q.samples_per_pixel, sums)
    want_sums, (want_prev, want_m2) = whole_fold
    assert np.array_equal(sums, want_sums) and sums.any()
    prev, m2 = A.fold(sums, np.zeros_like(sums), np.zeros(sums.shape, np.float64), tile_n, n)
    assert prev.tobytes() == want_prev.tobytes() and m2.tobytes() == want_m2.tobytes()
    act = A.active_mask(q.width, q.height, tile_n)
    assert (m2[~act] == 0).all() and (prev[~act] == 0).all() and (sums[~act] == 0).all() and m2[act].any()
