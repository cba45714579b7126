"""-m gpu: the HIP megakernel, called through the C ABI, against the oracle.

Exact tier: same seed => every sample takes the same path (equal draw counts),
per-pixel |dRGB| < 1e-4 (north_star's stated f32 tolerance; observed ~1e-6).  Plus bit-exact
host/device arithmetic, tile-partition invariance, determinism, error codes, and properties at
the BASELINE sizes."""
import ctypes as C

import os

import numpy as np
import pytest

import special_scenes
from vecchio_amd import DeviceScene, HostScene, ffi

pytestmark = pytest.mark.gpu

TOL = 1e-4   # north_star: per-pixel f32 RGB delta vs the seeded CPU reference

BUILDER_SCENES = ["random_spheres_iow", "cornell_box", "final_scene", "random_spheres_demo", "perlin_demo", "balls_demo", "bowser_demo",
                  "random_spheres_iow+sah", "final_scene+sah"]


def device_samples(ds, cam, p):
    lib = ds._lib             # (a scene belongs to the library that created it: the product, or the debug build of the same sources)
    lib.vk_debug_render_samples.restype = C.c_int
    lib.vk_debug_render_samples.argtypes = [C.c_void_p, C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_void_p, C.c_void_p]
    img = np.zeros((p.height, p.width, 3), np.float32)
    ps = np.zeros((p.width * p.height * p.samples_per_pixel, 4), np.float32)
    st = lib.vk_debug_render_samples(ds._h, C.byref(cam), C.byref(p), img.ctypes.data, ps.ctypes.data)
    assert st == 0, lib.vk_last_error().decode()
    return img, ps


def compare_samples(ps_o, ps_d, img_o, img_d):
    d_o, d_d = ps_o[:, 3].view(np.uint32), ps_d[:, 3].view(np.uint32)
    assert np.array_equal(d_o, d_d), f"{int((d_o != d_d).sum())} samples took a different path on the GPU"
    fo, fd = np.isfinite(ps_o[:, :3]).all(1), np.isfinite(ps_d[:, :3]).all(1)
    assert np.array_equal(fo, fd)
    rel = np.abs(ps_o[fo, :3] - ps_d[fo, :3]) / (np.abs(ps_o[fo, :3]) + 1e-3)
    assert rel.max() < 2e-5
    assert (np.abs(img_o - img_d) / np.maximum(1.0, np.abs(img_o))).max() < TOL      # (relative for pixels brighter than 1)


def test_device_arithmetic_is_bit_identical_to_host(device, oracle):
    lib = ffi.load_debug_lib()            # (the probe kernel lives in the debug build of the same sources, same compiler flags)
    rng = np.random.default_rng(11)
    n = 1 << 18
    a = np.concatenate([rng.uniform(-1e4, 1e4, n // 2), rng.uniform(-1, 1, n // 2)]).astype(np.float32)
    b = rng.normal(size=n).astype(np.float32)

    def dev(op, x, y):
        out = np.empty_like(x)
        assert lib.vk_debug_math(0, op, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size) == 0, lib.vk_last_error()
        return out

    for op in (0, 1, 4, 5):                               # sin, cos, atan2, pow5
        assert np.array_equal(dev(op, a, b).view(np.uint32), oracle.math(op, a, b).view(np.uint32)), f"op {op}"
    u = (rng.integers(0, 1 << 24, n).astype(np.float32)) * np.float32(2.0 ** -24)
    assert np.array_equal(dev(2, u, b).view(np.uint32), oracle.math(2, u, b).view(np.uint32))           # ln of 24-bit draws
    c = rng.uniform(-1.0000001, 1.0000001, n).astype(np.float32)
    assert np.array_equal(dev(3, c, b).view(np.uint32), oracle.math(3, c, b).view(np.uint32))           # asin incl. NaN domain
    # IEEE division / sqrt correctly rounded on the device; a*b+a NOT fused (-ffp-contract=off)
    assert np.array_equal(dev(6, a, b), (a / b).astype(np.float32))
    pos = np.abs(a)
    assert np.array_equal(dev(7, pos, b), np.sqrt(pos))
    assert np.array_equal(dev(9, a, b), (a * b).astype(np.float32) + a)


def test_device_math_equals_host_over_the_domain(device, oracle):
    """The inputs of tests/test_math_domain.py on the device, bit for bit against the host's build of the same header (the oracle):
    the stride-61 sweep of all 2^32 bit patterns, the special values, the samplers' angles, the neighbourhood of the reduction
    switch at +-2^22, asin near +-1, the ln ranges, and for atan2 the random bit-pattern pairs, the C99 special pairs and the
    extreme ratios; sincos (ops 11 / 12) and the samplers' bounded sincos (13 / 14, on its domain [+0, 2^22)) included.  Then the
    device directly against the correctly rounded reference on a sample of each, so that a common-mode change cannot hide behind
    the equality."""
    from concurrent.futures import ThreadPoolExecutor

    import math_domain as MD
    lib = ffi.load_debug_lib()

    def dev(op, x, y=None):
        x = np.ascontiguousarray(x, np.float32)
        y = np.zeros_like(x) if y is None else np.ascontiguousarray(y, np.float32)
        assert 0 < x.size <= 1 << 24
        out = np.empty_like(x)
        assert lib.vk_debug_math(0, op, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size) == 0, lib.vk_last_error()
        return out

    # (a, b) = the arguments of the probe: unary ops read a; atan2 is atan2(a, b)
    ya, xa = MD.atan2_random_pairs(1 << 22, seed=21)
    pairs = [(ya, xa), MD.atan2_special_pairs(), MD.atan2_extreme_pairs()]
    jobs = [(x, None, (0, 1, 2, 3, 5, 11, 12)) for x in list(MD.sweep_chunks()) + [MD.specials(), MD.switch_neighbourhood(),
            MD.asin_near_one()] + list(MD.sampler_angles()) + list(MD.log_ranges())] + [(a, b, (4,)) for a, b in pairs]

    def host(job):
        a, b, ops = job
        return [oracle.math(op, a, b) for op in ops]

    n = 0
    width = max(1, min(16, len(os.sched_getaffinity(0))))
    with ThreadPoolExecutor(width) as pool:
        for g in range(0, len(jobs), width):                     # (a group at a time: bounded memory)
            group = jobs[g:g + width]
            for (a, b, ops), want in zip(group, pool.map(host, group)):
                for op, w in zip(ops, want):
                    d = ~MD.same(dev(op, a, b), w)
                    assert not d.any(), f"op {op}: {int(d.sum())} of {a.size} device results differ from the host's, e.g. at {a[d][:4]}"
                    n += a.size
                x = a[(a >= 0) & (a < 2.0 ** 22) & ~np.signbit(a)]
                if b is None and x.size:                         # the samplers' sincos on its domain, against sinf_ / cosf_
                    assert np.array_equal(dev(13, x).view(np.uint32), dev(0, x).view(np.uint32))
                    assert np.array_equal(dev(14, x).view(np.uint32), dev(1, x).view(np.uint32))
    assert n > 7 * 70_000_000
    # the device against the correctly rounded reference itself: every 16th chunk of the sweep, the specials, the switch
    sample = [np.concatenate(list(MD.sweep_chunks())[::16]), MD.specials(), MD.switch_neighbourhood()]
    for fn in MD.UNARY:
        for x in sample:
            assert MD.same(dev(MD.OP[fn], x), MD.correctly_rounded(fn, x)).all(), fn
    for a, b in pairs:
        assert MD.same(dev(4, a, b), MD.correctly_rounded("atan2", a, b)).all()


def test_quotients_by_a_shared_reciprocal_are_the_divisions(device):
    """vk_trace.h div_by_a: the sphere test's n / |d|^2 from a reciprocal refined once and two fma corrections, in the range it is used
    in (|d|^2 in 3e-12 .. 3e12, |n| < 2^54, quotients down to far below tmin): 2^26 pairs, every one the correctly rounded quotient."""
    lib = ffi.load_debug_lib()
    rng = np.random.default_rng(12)
    n = 1 << 22
    bad = 0
    for rep in range(16):
        den = np.exp(rng.uniform(np.log(3e-12), np.log(3e12), n)).astype(np.float32)
        mag = np.exp(rng.uniform(np.log(1e-20), np.log(1.8e16), n))
        num = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        if rep % 4 == 1:                                   # quotients near 1 and near tmin, where a decision hangs on the last bit
            num = (den.astype(np.float64) * rng.choice([1.0, 1e-3, 0.5, 7.0], n) * (1.0 + rng.uniform(-1e-6, 1e-6, n))).astype(np.float32)
        if rep % 4 == 2:                                   # |d|^2 of unit-ish directions, numerators of ordinary scenes
            den = rng.uniform(0.2, 4.0, n).astype(np.float32); num = rng.uniform(-60.0, 60.0, n).astype(np.float32)
        out = np.empty_like(num)
        assert lib.vk_debug_math(0, 10, num.ctypes.data, den.ctypes.data, out.ctypes.data, n) == 0, lib.vk_last_error()
        want = (num / den).astype(np.float32)
        normal = np.abs(want) >= np.float32(1.2e-38)       # (a denormal quotient is far below tmin: its last bits decide nothing)
        bad += int((out[normal].view(np.uint32) != want[normal].view(np.uint32)).sum())
        assert (np.abs(out[~normal]) < np.float32(1e-30)).all()
    assert bad == 0, bad


@pytest.mark.parametrize("name", BUILDER_SCENES)
def test_builder_scene_per_sample(name, device, oracle, host_scenes):
    hs, cam = host_scenes(name)
    p = hs.params(72, 8, 50)
    ds = DeviceScene(hs.desc)
    img_d, ps_d = device_samples(ds, cam, p)
    img_o, ps_o = oracle.render_samples(hs.desc, cam, p)
    compare_samples(ps_o, ps_d, img_o, img_d)
    ds.close()


@pytest.mark.parametrize("name", sorted(special_scenes.ALL))
def test_special_scene_per_sample(name, device, oracle):
    d, desc, cam, p = special_scenes.ALL[name]()
    ds = DeviceScene(desc)
    img_d, ps_d = device_samples(ds, cam, p)
    img_o, ps_o = oracle.render_samples(desc, cam, p)
    compare_samples(ps_o, ps_d, img_o, img_d)
    ds.close()


@pytest.mark.parametrize("seed", range(16))
def test_random_scene_graph_per_sample(seed, device, oracle):
    """the randomised scene graphs of tests/test_fuzz_scenes.py through the C ABI"""
    from test_fuzz_scenes import Gen
    desc, cam, p = Gen(2000 + seed).build()
    ds = DeviceScene(desc)
    img_d, ps_d = device_samples(ds, cam, p)
    img_o, ps_o = oracle.render_samples(desc, cam, p)
    compare_samples(ps_o, ps_d, img_o, img_d)
    ds.close()


def test_sample_chunking_and_odd_sizes(device, oracle, host_scenes):
    """spp > 256 splits pixels into sample chunks (partial sums + resolve); odd image sizes give edge tiles"""
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    p = hs.params(37, 600, 30, height=29)
    img_d, _ = ds.render(cam, p)
    img_o, _ = oracle.render(hs.desc, cam, p)
    assert np.abs(img_o - img_d).max() < TOL
    ds.close()


def test_tile_partition_and_determinism(device, host_scenes):
    hs, cam = host_scenes("random_spheres_iow")
    ds = DeviceScene(hs.desc)
    p = hs.params(200, 300, 50)                           # 2 chunks
    full, st = ds.render(cam, p)
    again, _ = ds.render(cam, p)
    assert np.array_equal(full, again)                    # deterministic run to run
    for world in (2, 8):
        acc = np.zeros_like(full)
        for r in range(world):
            pr = hs.params(200, 300, 50, tile_rank=r, tile_world=world)
            ds.render(cam, pr, out=acc)
        assert np.array_equal(acc, full), f"{world}-way tile partition changed pixel values"
    ds.close()
    # the heavy-first tile order (probe launch + bucket sort) only decides who renders a tile when
    # (diagnostic switches are read once per scene, at creation)
    os.environ["VK_TILE_ORDER"] = "0"
    try:
        ds2 = DeviceScene(hs.desc)
    finally:
        del os.environ["VK_TILE_ORDER"]
    raster, _ = ds2.render(cam, p)
    assert np.array_equal(raster, full), "tile order changed pixel values"
    ds2.close()


def test_to_color_matches_reference_quantisation(device, host_scenes):
    import torch
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    p = hs.params(64, 16, 20)
    fb = torch.zeros((p.height, p.width, 3), dtype=torch.float32, device="cuda")
    ds.render_device(cam, p, fb.data_ptr())
    rgb8 = torch.zeros((p.height, p.width, 3), dtype=torch.uint8, device="cuda")
    ds.to_color_device(fb.data_ptr(), p.width, p.height, rgb8.data_ptr())
    torch.cuda.synchronize()
    host = fb.cpu().numpy()
    want = np.zeros((p.height, p.width, 3), np.uint8)
    ffi.load_host_lib().vkh_to_color(host.ctypes.data, p.width, p.height, want.ctypes.data)
    assert np.array_equal(rgb8.cpu().numpy(), want)
    ds.close()


def test_error_codes(device, host_scenes):
    hs, cam = host_scenes("cornell_box")
    ds = DeviceScene(hs.desc)
    lib = device
    out = np.zeros((8, 8, 3), np.float32)
    st = ffi.Stats()

    def status(p, c=cam):
        return lib.vk_render(ds._h, C.byref(c), C.byref(p), out.ctypes.data, C.byref(st))

    assert status(hs.params(1, 4, 10, height=8)) == ffi.VK_ERR_BAD_ARG            # width-1 == 0 divisor
    assert status(hs.params(8, 0, 10, height=8)) == ffi.VK_ERR_BAD_ARG
    bad = ffi.Camera.from_buffer_copy(cam)
    bad.time1 = bad.time0
    assert status(hs.params(8, 4, 10, height=8), bad) == ffi.VK_ERR_BAD_ARG       # gen_range(time0,time1) would panic
    p = hs.params(8, 4, 10, height=8, tile_rank=3, tile_world=2)
    assert status(p) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_render(None, C.byref(cam), C.byref(hs.params(8, 4, 10, height=8)), out.ctypes.data, None) == ffi.VK_ERR_BAD_ARG
    assert b"" != lib.vk_last_error()
    h = C.c_void_p()
    assert lib.vk_scene_create(hs.desc, 99, C.byref(h)) == ffi.VK_ERR_BAD_ARG
    ds.close()


def test_full_frame_per_sample_c2(device, oracle, host_scenes):
    """BASELINE C2 at full 1920x1080 (the headline config), every pixel: 4 spp = 8.3 M samples, each compared with
    the oracle — equal draw counts (same path) and |dRGB| < 1e-4 per pixel — plus determinism under an 8-way tile
    split at 32 spp."""
    hs, cam = host_scenes("random_spheres_iow")
    ds = DeviceScene(hs.desc)
    p = hs.params(1920, 4, 50)
    assert p.height == 1080
    img_d, ps_d = device_samples(ds, cam, p)
    img_o, ps_o = oracle.render_samples(hs.desc, cam, p)
    compare_samples(ps_o, ps_d, img_o, img_d)
    del ps_d, ps_o
    p = hs.params(1920, 32, 50)
    img, st = ds.render(cam, p)
    assert st.scene_in_lds == 1 and st.samples == 1920 * 1080 * 32
    assert np.isfinite(img).all() and img.min() >= 0.0
    acc = np.zeros_like(img)
    for r in range(8):
        ds.render(cam, hs.params(1920, 32, 50, tile_rank=r, tile_world=8), out=acc)
    assert np.array_equal(acc, img)
    ds.close()


def test_c1_full_spp_every_pixel(device, oracle, host_scenes):
    """BASELINE C1 exactly — InOneWeekend random spheres 400x225, 100 spp, depth 50 — the one config small enough for the
    oracle to render in full: every pixel of the HIP frame at the FULL spp against the oracle (9 M samples)."""
    hs, cam = host_scenes("random_spheres_iow")
    ds = DeviceScene(hs.desc)
    p = hs.params(400, 100, 50)
    assert (p.width, p.height) == (400, 225)
    img, st = ds.render(cam, p)
    ds.close()
    ref, cnt = oracle.render(hs.desc, cam, p)
    assert st.samples == cnt.samples == 400 * 225 * 100
    assert np.isfinite(img).all()
    assert np.abs(img - ref).max() < TOL


def sparse_oracle(oracle, desc, cam, p_full, hs, rank, world, threads=None):
    """oracle render of the tiles t with t % world == rank only; returns (image with -1 elsewhere, mask)"""
    po = hs.params(p_full.width, p_full.samples_per_pixel, p_full.max_depth, seed=p_full.seed, height=p_full.height, tile_rank=rank, tile_world=world)
    ref = np.full((p_full.height, p_full.width, 3), -1.0, np.float32)
    stt = oracle.load().oracle_render(desc, C.byref(cam), C.byref(po), ref.ctypes.data, threads or min(len(os.sched_getaffinity(0)), 32), None)
    assert stt == 0
    return ref, ref[..., 0] >= 0


def test_full_size_c5_stress_spheres(device, oracle, built):
    """BASELINE C5 geometry: 1 M procedurally placed spheres (stress_spheres:500, 2 M-item BVH traversed from global
    memory), full 4096x4096 frame at 1 spp: a sparse tile subset (every 257th tile, 65 K pixels all over the frame)
    per pixel against the oracle; the whole frame finite, non-negative and invariant under a 4-way tile split."""
    hs = HostScene("stress_spheres:500", 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    assert ds.info().lds_bytes == 0 and ds.info().n_prims >= 990000
    p = hs.params(4096, 1, 50)
    assert p.height == 4096
    img, st = ds.render(cam, p)
    assert st.scene_in_lds == 0 and st.samples == 4096 * 4096
    assert np.isfinite(img).all() and img.min() >= 0.0
    ref, mask = sparse_oracle(oracle, hs.desc, cam, p, hs, 5, 257)
    assert mask.sum() > 60000
    assert np.abs(img[mask] - ref[mask]).max() < TOL
    acc = np.zeros_like(img)
    for r in range(4):
        ds.render(cam, hs.params(4096, 1, 50, tile_rank=r, tile_world=4), out=acc)
    assert np.array_equal(acc, img)
    ds.close()
    hs.close()


def test_full_size_properties_c4_c3(device, oracle, host_scenes):
    """C4 (Cornell 1024x1024) and C3 (final scene 800x800) at full resolution, reduced spp: a band of
    rows compared pixel-exactly with the oracle, whole image finite."""
    for name, w in (("cornell_box", 1024), ("final_scene", 800)):
        hs, cam = host_scenes(name)
        ds = DeviceScene(hs.desc)
        p = hs.params(w, 4, 50)
        img, _ = ds.render(cam, p)
        assert np.isfinite(img).all() and img.min() >= 0.0
        # oracle on tiles of one 8-row band only (tile partition = every (w/8)-th... use rank/world to pick a sparse subset)
        ref, mask = sparse_oracle(oracle, hs.desc, cam, p, hs, 7, 61)
        assert mask.sum() > 1000
        assert np.abs(img[mask] - ref[mask]).max() < TOL
        ds.close()
