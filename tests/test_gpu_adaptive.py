"""-m gpu: adaptive progressive rendering (vk_progress_set_adaptive).  Converged tiles stop; every pixel of tile t is still, bit for
bit, vk_render's pixel at samples_per_pixel = N_t (the tile's own count), and every decision of the device's judge is reproduced by
tests/adaptive_ref.py from the raw moments.  Plus partitions, devices, the error estimate, the exact re-treeing fallback, full
convergence, invalid calls, and the scene's own later behaviour (dual launch, tree verdicts)."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as R
from vecchio_amd import DeviceScene, HostScene, ffi

pytestmark = pytest.mark.gpu

SCENES = [("cornell_box", 48), ("random_spheres_iow", 96), ("final_scene_nextweek", 48)]
BUDGET, WINDOW = 64, 8


def with_spp(p, spp):
    q = ffi.RenderParams.from_buffer_copy(p)
    q.samples_per_pixel = spp
    return q


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


_scenes = {}


def scene(name, width):
    if (name, width) not in _scenes:
        hs = HostScene(name, 1)
        _scenes[(name, width)] = (hs, hs.next_camera(), DeviceScene(hs.desc))
    return _scenes[(name, width)]


_tols = {}


def tolerance(name, width):
    """an abs_tol that freezes some tiles but not all within the budget: the median over tiles of the largest per-pixel standard error
    after half the budget (a non-adaptive handle of the same frame)"""
    if (name, width) not in _tols:
        hs, cam, ds = scene(name, width)
        p = hs.params(width, BUDGET, 50)
        with ds.progress(cam, p, stderr=True) as pr:
            for _ in range(BUDGET // WINDOW // 2):
                pr.step(WINDOW)
            se = pr.stderr().max(axis=2)
        h, w = se.shape
        tx, ty = R.tile_grid(w, h)
        pad = np.zeros((ty * 8, tx * 8), np.float32)
        pad[:h, :w] = se
        _tols[(name, width)] = float(np.median(pad.reshape(ty, 8, tx, 8).max(axis=(1, 3))))
    return _tols[(name, width)]


def adaptive(name, width, min_steps=2):
    return dict(abs_tol=tolerance(name, width), rel_tol=0.0, min_samples=0, min_steps=min_steps)


def tile_image(tmap, width, height):
    return np.repeat(np.repeat(tmap, 8, 0), 8, 1)[:height, :width]


def rows_up(img, p):
    """an RGB8 image (top row first) as y up, like the tile map"""
    return img[::-1] if p.output_format == ffi.VK_OUTPUT_RGB8 else img


def check_exact(ds, cam, p, img, tmap):
    """every pixel equals vk_render's at its tile's count (pixels of tiles outside the partition: not compared)"""
    per_px = tile_image(tmap, p.width, p.height)
    up = rows_up(img, p)
    for n in np.unique(tmap):
        if n == 0:
            continue
        ref, st = ds.render(cam, with_spp(p, int(n)))
        assert st.clamped_samples == 0
        sel = per_px == n
        bad = int((bits(up[sel]) != bits(rows_up(ref, p)[sel])).any(-1).sum())
        assert bad == 0, f"N = {n}: {bad} pixels differ from vk_render"


@pytest.mark.parametrize("fmt", [ffi.VK_OUTPUT_F32, ffi.VK_OUTPUT_RGB8])
@pytest.mark.parametrize("name,width", SCENES)
def test_every_tile_is_vk_render_at_its_own_count(name, width, fmt, device):
    hs, cam, ds = scene(name, width)
    p = hs.params(width, BUDGET, 50, output_format=fmt)
    with ds.progress(cam, p, adaptive=adaptive(name, width)) as pr:
        for _ in range(BUDGET // WINDOW):
            img, _ = pr.step(WINDOW)
        tmap, inf = pr.tile_samples()
        assert pr.info().clamped_samples == 0
    assert 0 < inf.tiles_active < inf.tiles_total == tmap.size, (inf.tiles_active, inf.tiles_total)
    assert (tmap < BUDGET).any() and (tmap == BUDGET).any()
    check_exact(ds, cam, p, img, tmap)


@pytest.mark.parametrize("name,width", SCENES)
def test_decisions_match_the_reference(name, width, device):
    """after every step the moments and the numpy judge give the library's map; frozen tiles keep their count and their pixels"""
    hs, cam, ds = scene(name, width)
    p = hs.params(width, BUDGET, 50)
    ap = adaptive(name, width)
    tx, ty = R.tile_grid(p.width, p.height)
    tile_n = np.zeros((ty, tx), np.uint32)           # the reference's map: frozen count, 0 = active
    prev_img = None
    with ds.progress(cam, p, adaptive=ap) as pr:
        for j in range(1, BUDGET // WINDOW + 1):
            img, st = pr.step(WINDOW)
            done = j * WINDOW
            run, m2 = pr.moments()
            frozen = R.judge(run, m2, tile_n, done, j, ap["abs_tol"], ap["rel_tol"], ap["min_samples"], ap["min_steps"])
            was_frozen = tile_n != 0
            tile_n = np.where(frozen, done, tile_n).astype(np.uint32)
            tmap, inf = pr.tile_samples()
            assert np.array_equal(tmap, np.where(tile_n != 0, tile_n, done)), f"step {j}: the maps differ"
            assert inf.tiles_active == int((tile_n == 0).sum()), f"step {j}"
            assert inf.samples_rendered == int((tmap.astype(np.int64) * R.tile_pixels(p.width, p.height)).sum())
            if prev_img is not None:
                keep = tile_image(was_frozen, p.width, p.height)
                assert np.array_equal(bits(img[keep]), bits(prev_img[keep])), f"step {j}: a frozen tile's pixels changed"
            prev_img = img.copy()
            assert st.samples == int((np.where(was_frozen, 0, 1) * R.tile_pixels(p.width, p.height)).sum()) * WINDOW
    assert 0 < int((tile_n != 0).sum()) < tile_n.size


def test_partitions_and_devices(device):
    name, width = "cornell_box", 48
    hs, cam, ds = scene(name, width)
    ap = adaptive(name, width)
    p = hs.params(width, BUDGET, 50, output_format=ffi.VK_OUTPUT_RGB8)
    with ds.progress(cam, p, adaptive=ap) as pr:
        for _ in range(BUDGET // WINDOW):
            full, _ = pr.step(WINDOW)
        fmap, finf = pr.tile_samples()
    assert 0 < finf.tiles_active < finf.tiles_total
    union, umap = np.full_like(full, 77), np.zeros_like(fmap)
    for rank in range(3):
        pr_p = hs.params(width, BUDGET, 50, tile_rank=rank, tile_world=3, output_format=ffi.VK_OUTPUT_RGB8)
        own = np.full_like(full, 77)
        with ds.progress(cam, pr_p, adaptive=ap) as pr:
            for _ in range(BUDGET // WINDOW):
                pr.step(WINDOW, out=own)
            m, inf = pr.tile_samples()
        mine = R.partition_mask(p.width, p.height, rank, 3)
        assert not m[~mine].any() and inf.tiles_total == int(mine.sum())
        umap[mine] = m[mine]
        sel = rows_up(tile_image(mine, p.width, p.height), p)
        assert (own[~sel] == 77).all(), f"rank {rank} wrote another partition's pixels"
        union[sel] = own[sel]
    assert np.array_equal(umap, fmap) and np.array_equal(union, full)
    lists = [[0, 0]]
    if device.vk_device_count() > 1:
        lists.append(list(range(device.vk_device_count())))
    pf = hs.params(width, BUDGET, 50)
    with ds.progress(cam, pf, adaptive=ap) as pr:
        for _ in range(BUDGET // WINDOW):
            one, _ = pr.step(WINDOW)
        omap, _ = pr.tile_samples()
    for devs in lists:
        dm = DeviceScene(hs.desc, devices=devs)
        try:
            with dm.progress(cam, pf, adaptive=ap) as pr:
                for _ in range(BUDGET // WINDOW):
                    img, _ = pr.step(WINDOW)
                m, _ = pr.tile_samples()
            assert np.array_equal(m, omap), f"devices {devs}: maps differ"
            assert np.array_equal(bits(img), bits(one)), f"devices {devs}: images differ"
        finally:
            dm.close()


def test_stderr_uses_each_tiles_own_count(device):
    name, width = "cornell_box", 48
    hs, cam, ds = scene(name, width)
    p = hs.params(width, BUDGET, 50)
    with ds.progress(cam, p, adaptive=adaptive(name, width)) as pr:
        for _ in range(BUDGET // WINDOW):
            pr.step(WINDOW)
        tmap, inf = pr.tile_samples()
        run, m2 = pr.moments()
        se = pr.stderr()
    assert 0 < inf.tiles_active < inf.tiles_total
    want = R.stderr(run, m2, tmap, tmap // WINDOW)              # (equal windows: k_t = N_t / 8)
    assert np.array_equal(se, want), f"{int((se != want).sum())} components differ, worst {float(np.abs(se - want).max())}"


def test_fallback_in_a_later_window_keeps_frozen_tiles(device, monkeypatch):
    name, width = "random_spheres_iow", 96
    hs, cam, plain = scene(name, width)
    p = hs.params(width, BUDGET, 50)
    ap = adaptive(name, width)
    with plain.progress(cam, p, adaptive=ap) as pr:
        for n in (8, 8, 48):
            want, _ = pr.step(n)
        want_map, _ = pr.tile_samples()
    monkeypatch.setenv("VK_REDO_REGION_CAP", "1")
    ds = DeviceScene(hs.desc)
    monkeypatch.delenv("VK_REDO_REGION_CAP")
    try:
        assert ds.info().tree != ffi.VK_TREE_HANDED_OVER
        overflowed = []
        with ds.progress(cam, p, adaptive=ap) as pr:
            for n in (8, 8, 48):
                img, s = pr.step(n)
                overflowed.append(ds.last_requeued_samples() == s.samples)
            tmap, inf = pr.tile_samples()
        assert overflowed[2], f"the third window did not overflow its queues: {overflowed}"
        assert 0 < inf.tiles_active < inf.tiles_total
        assert np.array_equal(tmap, want_map) and np.array_equal(bits(img), bits(want))
        check_exact(plain, cam, p, img, tmap)
    finally:
        ds.close()


def test_full_convergence_is_a_no_op(device):
    hs, cam, ds = scene("cornell_box", 48)
    p = hs.params(48, BUDGET, 50)
    with ds.progress(cam, p, adaptive=dict(abs_tol=1e30, rel_tol=0.0, min_samples=0, min_steps=2)) as pr:
        pr.step(WINDOW)
        img, _ = pr.step(WINDOW)
        img = img.copy()
        tmap, inf = pr.tile_samples()
        assert inf.tiles_active == 0 and (tmap == 2 * WINDOW).all()
        again, st = pr.step(WINDOW)
        assert st.samples == 0 and np.array_equal(bits(again), bits(img))
        m2, inf2 = pr.tile_samples()
        assert np.array_equal(m2, tmap) and pr.info().samples_done == 3 * WINDOW
        assert inf2.samples_rendered == int((tmap.astype(np.int64) * R.tile_pixels(48, p.height)).sum())
    check_exact(ds, cam, p, again, tmap)


def test_invalid_calls_change_nothing(device):
    hs, cam, ds = scene("cornell_box", 48)
    p = hs.params(48, BUDGET, 50)
    lib = ds._lib
    good = ffi.AdaptiveParams(1e-3, 0.0, 0, 2)
    assert lib.vk_progress_set_adaptive(None, C.byref(good)) == ffi.VK_ERR_BAD_ARG
    with ds.progress(cam, p) as pr:                                            # no VK_PROGRESS_STDERR
        assert lib.vk_progress_set_adaptive(pr._h, C.byref(good)) == ffi.VK_ERR_BAD_ARG
        assert pr.tile_samples()[1].tiles_active == pr.tile_samples()[1].tiles_total
    ap = adaptive("cornell_box", 48)
    with ds.progress(cam, p, adaptive=ap) as pr:
        for bad in (ffi.AdaptiveParams(1e-3, 0.0, 0, 1), ffi.AdaptiveParams(-1.0, 0.0, 0, 2), ffi.AdaptiveParams(0.0, -1e-3, 0, 2),
                    ffi.AdaptiveParams(float("nan"), 0.0, 0, 2), ffi.AdaptiveParams(0.0, float("inf"), 0, 2)):
            assert lib.vk_progress_set_adaptive(pr._h, C.byref(bad)) == ffi.VK_ERR_BAD_ARG
        for _ in range(BUDGET // WINDOW):
            img, _ = pr.step(WINDOW)
        first_map, _ = pr.tile_samples()
        first = img.copy()
        assert lib.vk_progress_set_adaptive(pr._h, C.byref(good)) == ffi.VK_ERR_BAD_ARG      # after a step
        assert np.array_equal(pr.tile_samples()[0], first_map)
        pr.reset()                                                             # every tile active again, the parameters kept
        m, inf = pr.tile_samples()
        assert inf.tiles_active == inf.tiles_total and not m.any()
        for _ in range(BUDGET // WINDOW):
            img, _ = pr.step(WINDOW)
        assert np.array_equal(pr.tile_samples()[0], first_map) and np.array_equal(bits(img), bits(first))


def test_the_scenes_later_behaviour_is_untouched(device, monkeypatch):
    """an adaptive progress ending with few active tiles does not strike the scene's dual launch off or suspend its tree"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = -(-cus * 112 // 24)
    width, height = 320, 8 * -(-tiles // 40)
    hs = HostScene("random_spheres_iow", 1)
    cam = hs.next_camera()
    monkeypatch.setenv("VK_CHUNK_CAP", "1")          # (a unit per tile and sample: the dual launch's threshold at a small size)
    ds = DeviceScene(hs.desc)
    monkeypatch.delenv("VK_CHUNK_CAP")
    try:
        p = hs.params(width, 96, 50, height=height)
        roles = lambda: sorted(r.role for r in ffi.last_launches(ds._lib, ds._h) if r.role in (ffi.VK_LAUNCH_MAIN, ffi.VK_LAUNCH_DUAL_1024,
                                                                                              ffi.VK_LAUNCH_DUAL_768))
        keys = lambda: [(r.role, r.features, r.lds_scene, r.minw, r.cost, r.grid_form, r.block_size) for r in
                        ffi.last_launches(ds._lib, ds._h)]
        ds.render(cam, with_spp(p, 24))
        assert roles() == [ffi.VK_LAUNCH_DUAL_1024, ffi.VK_LAUNCH_DUAL_768]
        suspended = ds.info().tree_suspended_frames
        with ds.progress(cam, p, stderr=True) as pr:
            pr.step(24)
            plain_keys = keys()
            pr.step(24)
            se = pr.stderr().max(axis=2)
        tile_se = se.reshape(height // 8, 8, width // 8, 8).max(axis=(1, 3))
        tol = float(np.quantile(tile_se, 0.9))       # nine tiles in ten converge after two windows
        with ds.progress(cam, p, adaptive=dict(abs_tol=tol, rel_tol=0.0, min_samples=0, min_steps=2)) as pr:
            pr.step(24)
            assert keys() == plain_keys               # the same instances and shapes as a non-adaptive window
            pr.step(24)
            inf = pr.tile_samples()[1]
            assert 0 < inf.tiles_active < inf.tiles_total // 4, (inf.tiles_active, inf.tiles_total)
            for _ in range(2):
                img, _ = pr.step(24)
            tmap, inf = pr.tile_samples()
        check_exact(ds, cam, p, img, tmap)
        ds.render(cam, with_spp(p, 24))
        assert roles() == [ffi.VK_LAUNCH_DUAL_1024, ffi.VK_LAUNCH_DUAL_768], "the dual launch was struck off"
        assert ds.info().tree_suspended_frames == suspended
    finally:
        ds.close()
