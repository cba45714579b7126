"""-m gpu: progressive rendering (vk_progress_*, ABI 7).  Samples are keyed by their index and pixel sums are exact fixed point, so a
frame accumulated over sample windows is the one-shot frame BIT FOR BIT: after every step the image is vk_render's image at
samples_per_pixel = samples done (same seed), whatever the windows, the output format, the tile partition, the devices, the exact
re-treeing fallback or a vk_render of another view in between.  Plus the invalid calls, the batch-means error estimate and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from vecchio_amd import DeviceScene, HostScene, ffi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4


def with_spp(p, spp):
    q = ffi.RenderParams.from_buffer_copy(p)
    q.samples_per_pixel = spp
    return q


def windows(total, steps):
    """`steps` windows of (nearly) equal length adding up to `total`"""
    return [total * (i + 1) // steps - total * i // steps for i in range(steps)]


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def info_tuple(pr):
    i = pr.info()
    return (i.samples_done, i.samples_budget, i.steps, i.flags, i.clamped_samples)


def moved(cam, dx):
    c = ffi.Camera.from_buffer_copy(cam)
    c.origin[0] += dx
    c.lower_left_corner[0] += dx
    return c


_scenes = {}


def scene(name, width, **kw):
    key = (name, width)
    if key not in _scenes:
        hs = HostScene(name, 1)
        cam = hs.next_camera()
        _scenes[key] = (hs, cam, DeviceScene(hs.desc, **kw))
    return _scenes[key]


SCENES = [("cornell_box", 48), ("random_spheres_iow", 96), ("final_scene_nextweek", 48)]


@pytest.mark.parametrize("name,width", SCENES)
def test_windows_add_up_to_the_frame_bit_for_bit(name, width, device):
    hs, cam, ds = scene(name, width)
    p = hs.params(width, 64, 50)
    ref, st = ds.render(cam, p)
    assert st.clamped_samples == 0
    for steps in (1, 7, 24, 32):
        with ds.progress(cam, p) as pr:
            total = 0
            for n in windows(64, steps):
                img, s = pr.step(n)
                total += s.samples
            assert np.array_equal(bits(img), bits(ref)), f"{name}, {steps} steps: {int((img != ref).any(2).sum())} pixels differ"
            assert total == st.samples
            i = pr.info()
            assert (i.samples_done, i.samples_budget, i.steps, i.clamped_samples) == (64, 64, steps, 0)


@pytest.mark.parametrize("name,width", SCENES[:2])
def test_every_intermediate_image_is_a_frame_of_its_own(name, width, device, oracle):
    hs, cam, ds = scene(name, width)
    p = hs.params(width, 64, 50)
    done = 0
    with ds.progress(cam, p) as pr:
        for k, n in enumerate(windows(64, 7)):
            img, s = pr.step(n)
            done += n
            ref, st = ds.render(cam, with_spp(p, done))
            assert st.clamped_samples == 0
            assert np.array_equal(bits(img), bits(ref)), f"{name} after {done} samples: {int((img != ref).any(2).sum())} pixels differ"
            if k == 2:
                o, _ = oracle.render(hs.desc, cam, with_spp(p, done))
                err = float(np.abs(img - o).max())
                assert err < TOL, f"{name} at {done} samples: max |dRGB| vs the oracle {err}"
        assert pr.info().clamped_samples == 0


def test_rgb8_over_tile_partitions(device):
    hs, cam, ds = scene("cornell_box", 48)
    full, _ = ds.render(cam, hs.params(48, 64, 50, output_format=ffi.VK_OUTPUT_RGB8))
    union = np.full_like(full, 77)
    tiles_x = (48 + 7) // 8
    for rank in range(3):
        p = hs.params(48, 64, 50, tile_rank=rank, tile_world=3, output_format=ffi.VK_OUTPUT_RGB8)
        own = np.full_like(full, 77)
        with ds.progress(cam, p) as pr:
            for n in windows(64, 5):
                pr.step(n, out=own)
        for row in range(p.height):
            y = p.height - 1 - row            # RGB8 rows are top-down
            for x in range(p.width):
                mine = ((y // 8) * tiles_x + x // 8) % 3 == rank
                if mine:
                    union[row, x] = own[row, x]
                else:
                    assert (own[row, x] == 77).all(), f"rank {rank} wrote pixel ({x}, {y}) of another partition"
    assert np.array_equal(union, full)


def test_multi_device_gives_the_single_device_image(device):
    hs, cam, ds = scene("cornell_box", 48)
    p = hs.params(48, 64, 50)
    with ds.progress(cam, p) as pr:
        for n in windows(64, 4):
            one, _ = pr.step(n)
    lists = [[0, 0]]
    n_dev = device.vk_device_count()
    if n_dev > 1:
        lists.append(list(range(n_dev)))
    for devs in lists:
        dm = DeviceScene(hs.desc, devices=devs)
        try:
            with dm.progress(cam, p) as pr:
                for n in windows(64, 4):
                    img, _ = pr.step(n)
                assert pr.info().samples_done == 64
            assert np.array_equal(bits(img), bits(one)), f"devices {devs}"
        finally:
            dm.close()


def test_fallback_mid_accumulation_keeps_earlier_windows(device, monkeypatch):
    """VK_REDO_REGION_CAP=1 leaves one entry per queue between the two launches of exact re-treeing: a window whose dropped samples do
    not fit is cleared and rendered again by the fallback launch.  That clears the WINDOW's sums only: the windows before it stay."""
    hs = HostScene("random_spheres_iow", 1)
    cam = hs.next_camera()
    p = hs.params(96, 64, 50)
    plain = DeviceScene(hs.desc)
    ref, _ = plain.render(cam, p)
    plain.close()
    monkeypatch.setenv("VK_REDO_REGION_CAP", "1")
    ds = DeviceScene(hs.desc)            # (the switch is read when a scene is created)
    monkeypatch.delenv("VK_REDO_REGION_CAP")
    try:
        assert ds.info().tree != ffi.VK_TREE_HANDED_OVER
        overflowed = []
        with ds.progress(cam, p) as pr:
            for n in (1, 63):
                img, s = pr.step(n)
                overflowed.append(ds.last_requeued_samples() == s.samples)     # (a frame that overflowed counts as entirely requeued)
        assert overflowed[1], f"the second window did not overflow its queues: {overflowed}"
        assert np.array_equal(bits(img), bits(ref)), f"{int((img != ref).any(2).sum())} pixels differ"
    finally:
        ds.close()


def test_interleaved_render_and_reset(device):
    hs, cam, ds = scene("cornell_box", 48)
    p = hs.params(48, 64, 50)
    cam2 = moved(cam, 40.0)
    ref, _ = ds.render(cam, p)
    ref2, _ = ds.render(cam2, p)
    assert not np.array_equal(ref, ref2)
    with ds.progress(cam, p) as pr:
        pr.step(20)
        other, _ = ds.render(cam2, with_spp(p, 16))        # another view between two steps, on the same scene
        img, _ = pr.step(44)
        assert np.array_equal(bits(img), bits(ref))
        pr.reset(cam2)
        assert info_tuple(pr)[:3] == (0, 64, 0)
        for n in windows(64, 3):
            img, _ = pr.step(n)
        assert np.array_equal(bits(img), bits(ref2))
        pr.reset()                                          # the same camera, from sample 0
        img, _ = pr.step(64)
        assert np.array_equal(bits(img), bits(ref2))


def test_invalid_calls_change_nothing(device):
    hs, cam, ds = scene("cornell_box", 48)
    p = hs.params(48, 64, 50)
    lib = ds._lib
    h = C.c_void_p()
    bad = with_spp(p, 64)
    bad.width = 1
    assert lib.vk_progress_create(ds._h, C.byref(cam), C.byref(bad), 0, C.byref(h)) == ffi.VK_ERR_BAD_ARG and not h.value
    bad = with_spp(p, 0)
    assert lib.vk_progress_create(ds._h, C.byref(cam), C.byref(bad), 0, C.byref(h)) == ffi.VK_ERR_BAD_ARG and not h.value
    with ds.progress(cam, p) as pr:
        first, _ = pr.step(10)
        first = first.copy()
        before = info_tuple(pr)
        img = np.zeros_like(first)
        assert lib.vk_progress_step(pr._h, 0, img.ctypes.data_as(C.c_void_p), None) == ffi.VK_ERR_BAD_ARG
        assert lib.vk_progress_step(pr._h, 55, img.ctypes.data_as(C.c_void_p), None) == ffi.VK_ERR_BAD_ARG      # 10 + 55 > 64
        assert lib.vk_progress_step(pr._h, 1, None, None) == ffi.VK_ERR_BAD_ARG
        assert lib.vk_progress_step_device(pr._h, 0, C.c_void_p(1), None, None) == ffi.VK_ERR_BAD_ARG
        assert lib.vk_progress_stderr(pr._h, img.ctypes.data_as(C.c_void_p)) == ffi.VK_ERR_BAD_ARG    # no VK_PROGRESS_STDERR
        badcam = ffi.Camera.from_buffer_copy(cam)
        badcam.time1 = badcam.time0
        assert lib.vk_progress_reset(pr._h, C.byref(badcam)) == ffi.VK_ERR_BAD_ARG
        assert not img.any()
        assert info_tuple(pr) == before
        rest, _ = pr.step(54)
        ref, _ = ds.render(cam, p)
        assert np.array_equal(bits(rest), bits(ref))
    with ds.progress(cam, p, stderr=True) as pr:
        pr.step(8)
        with pytest.raises(RuntimeError):
            pr.stderr()                                     # one step: no estimate yet
        assert info_tuple(pr) == (8, 64, 1, ffi.VK_PROGRESS_STDERR, 0)


def test_stderr_is_the_batch_means_estimate(device):
    """(a) deterministic: the library's estimate against a float64 recomputation from the returned images"""
    hs, cam, ds = scene("cornell_box", 48)
    p = hs.params(48, 64, 50)
    ws = windows(64, 16)
    sums, done = [np.zeros((p.height, p.width, 3))], 0
    with ds.progress(cam, p, stderr=True) as pr:
        for n in ws:
            img, _ = pr.step(n)
            done += n
            sums.append(img.astype(np.float64) * done)
        se = pr.stderr()
    n_j = np.array(ws, np.float64)[:, None, None, None]
    m_j = np.diff(np.stack(sums), axis=0) / n_j                 # every window's own mean
    N, k = float(done), len(ws)
    m = sums[-1] / N
    want = np.sqrt(np.maximum((n_j * m_j ** 2).sum(0) - N * m ** 2, 0.0) / ((k - 1) * N))
    ok = np.isclose(se, want, rtol=1e-3, atol=1e-5)
    assert ok.all(), f"{int((~ok).sum())} components off, worst {float(np.abs(se - want).max())}"
    assert se.max() > 1e-3       # (not all zero)


def test_stderr_agrees_with_the_spread_over_seeds(device):
    """(b) statistical: the InOneWeekend scene (sky light only: every sample in [0, 1], no fireflies) at 64 spp in 16 steps, 8 seeds — the
    standard deviation of the final mean over the seeds, averaged over the pixels, against the mean reported standard error"""
    hs, cam, ds = scene("random_spheres_iow", 96)
    finals, errs = [], []
    for seed in range(8):
        p = hs.params(96, 64, 50, seed=100 + seed)
        with ds.progress(cam, p, stderr=True) as pr:
            for n in windows(64, 16):
                img, _ = pr.step(n)
            finals.append(img.copy())
            errs.append(pr.stderr())
    spread = np.std(np.stack(finals), axis=0, ddof=1).mean()
    reported = np.stack(errs).mean()
    assert abs(reported / spread - 1.0) < 0.25, (reported, spread)


def test_cli_progressive_frame_is_byte_identical(device, tmp_path):
    from vecchio_amd import build
    cli = build.build_cli()
    build.build_device()
    a, b = tmp_path / "one", tmp_path / "four"
    a.mkdir()
    b.mkdir()
    subprocess.run([cli, "cornell_box", "100", "64", "20", "1", "1"], cwd=a, check=True, timeout=300, capture_output=True)
    r = subprocess.run([cli, "cornell_box", "100", "64", "20", "1", "1", "4"], cwd=b, check=True, timeout=300, capture_output=True,
                       text=True)
    assert (a / "output_0000.ppm").read_bytes() == (b / "output_0000.ppm").read_bytes()
    assert sorted(f.name for f in b.iterdir()) == ["output_0000.ppm"] + [f"output_0000_step{k:02d}.ppm" for k in range(4)]
    assert (b / "output_0000_step03.ppm").read_bytes() == (a / "output_0000.ppm").read_bytes()
    assert "64/64 samples" in r.stderr and "mean relative standard error" in r.stderr, r.stderr
