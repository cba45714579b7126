"""Specular guides (vk_render_guides) on the MI355X, through the C ABI: per sample against tests/guides_ref.py on the scenes of
tests/test_guides_emu.py (the CPU counterpart, which holds the scenes and the comparison); max_bounces = 0 against vk_render_aov bit for
bit; every view of a sphere-only world the walk runs on, each in a child process, bit for bit against the tree as handed over; tile
partitions, device pointers, non-interference with vk_render and a progress handle; and what the guides buy the denoiser on the frame
they were made for.  Run with -s for the figures."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aov_ref
import guides_ref
import test_guides_emu as shared
from test_gpu_aov import FORMS, FORM_W
from vecchio_amd import DeviceScene, HostScene, ffi

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDER_SCENES = ("random_spheres_iow", "cornell_box", "final_scene", "final_scene_nextweek", "random_spheres_demo", "perlin_demo", "balls_demo",
                  "bowser_demo")


def singles(ds, cam, p, samples, **guide):
    q = ffi.RenderParams()
    C.pointer(q)[0] = p
    q.samples_per_pixel = 1
    return [ds.render_guides(cam, q, first_sample=s, guide=ds.guide_params(**guide))[0] for s in samples]


def check(desc, cam, p, oracle, samples=shared.SAMPLES, **guide):
    ds = DeviceScene(desc)
    try:
        got = singles(ds, cam, p, samples, **guide)
    finally:
        ds.close()
    ref = guides_ref.ref_guides(oracle, desc, cam, p, samples, guide.get("max_bounces", 4), guide.get("fuzz_max", 0.0))
    w = shared.Worst()
    shared.check_per_sample(got, ref, p, w)
    print("\n   device vs reference:", w, " delta samples %d, mean bounces %.3f" % (int(ref["delta"].sum()), float(ref["bounces"].mean())))
    return ref


@pytest.mark.parametrize("name", shared.BUILDERS)
def test_builder_scene_per_sample(name, device, oracle, host_scenes):
    desc, cam, p = shared.builder(host_scenes, name)
    ref = check(desc, cam, p, oracle)
    assert ref["delta"].any()


@pytest.mark.parametrize("name", sorted(shared.HAND_BUILT))
def test_hand_built_scene_per_sample(name, device, oracle):
    d, desc, cam, p = shared.HAND_BUILT[name]()
    check(desc, cam, p, oracle)


@pytest.mark.parametrize("fuzz_max", [0.0, 0.5])
def test_fuzz_max_decides_what_is_a_mirror(fuzz_max, device, oracle):
    d, desc, cam, p = shared.rough_metal()
    check(desc, cam, p, oracle, fuzz_max=fuzz_max)


def test_bounce_cap_of_eight(device, oracle):
    d, desc, cam, p = shared.mirror_facing_mirror()
    p.width, p.height = 12, 8
    ref = check(desc, cam, p, oracle, samples=(0,), max_bounces=8)
    assert (ref["bounces"] == 8).any()


@pytest.mark.parametrize("seed", shared.FUZZ_SEEDS)
def test_fuzz_graph_per_sample(seed, device, oracle):
    desc, cam, p = shared.fuzz(seed)
    check(desc, cam, p, oracle)


def bits_equal(got, want, channels):
    for ch in channels:
        np.testing.assert_array_equal(got[ch].view(np.uint32), want[ch].view(np.uint32), err_msg=ch)


@pytest.mark.parametrize("name", BUILDER_SCENES)
def test_zero_bounces_is_vk_render_aov_bit_for_bit(name, device):
    hs = HostScene(name, 1)
    cam = hs.next_camera()
    p = hs.params(64, 4, 50, seed=7, height=40)
    ds = DeviceScene(hs.desc)
    try:
        want, _ = ds.render_aov(cam, p, first_sample=3)
        got, _ = ds.render_guides(cam, p, first_sample=3, guide=ds.guide_params(max_bounces=0))
        bits_equal(got, want, aov_ref.CHANNELS)
        assert (got["bounces"] == 0).all()
        # coverage is the primary ray's at any number of bounces
        full, _ = ds.render_guides(cam, p, first_sample=3)
        np.testing.assert_array_equal(full["coverage"].view(np.uint32), want["coverage"].view(np.uint32))
    finally:
        ds.close()
        hs.close()


def test_windows_aggregate_exactly(device, host_scenes):
    for name in ("random_spheres_iow", "cornell_box"):
        desc, cam, p = shared.builder(host_scenes, name)
        ds = DeviceScene(desc)
        try:
            one = singles(ds, cam, p, range(12))
            for lo, hi in ((0, 8), (4, 12)):
                q = ffi.RenderParams()
                C.pointer(q)[0] = p
                q.samples_per_pixel = hi - lo
                got, _ = ds.render_guides(cam, q, first_sample=lo)
                bits_equal(got, guides_ref.aggregate(one[lo:hi]), guides_ref.CHANNELS)
        finally:
            ds.close()


_FORM_CHILD = """
import sys, ctypes as C
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
from vecchio_amd import DeviceScene, HostScene, ffi
lib = ffi.load_debug_lib() if %(debug)r else None
res = {}
for flags in (0, ffi.VK_SCENE_REFERENCE_TREE):
    hs = HostScene(%(scene)r, %(seed)d); hs.desc.contents.flags = flags; cam = hs.next_camera()
    ds = DeviceScene(hs.desc, lib=lib) if lib is not None else DeviceScene(hs.desc)
    img, st = ds.render(cam, hs.params(128, 8, 50, seed=3))
    tree, in_lds = ds.info().tree, bool(st.scene_in_lds)
    got = ds.render_guides(cam, hs.params(%(w)d, 2, 50, seed=7, height=%(w)d), first_sample=1)[0]
    res[flags] = (tree, in_lds, got)
    ds.close(); hs.close()
tree, in_lds, got = res[0]
rtree, _, rgot = res[ffi.VK_SCENE_REFERENCE_TREE]
assert tree == ffi.%(tree)s and in_lds == %(in_lds)r, (tree, in_lds)
assert rtree == ffi.VK_TREE_HANDED_OVER, rtree
for ch in ("albedo", "normal", "depth", "coverage", "bounces"):
    assert np.array_equal(got[ch].view(np.uint32), rgot[ch].view(np.uint32)), ch
assert got["bounces"].max() >= 1
print("FORM OK", tree, in_lds)
"""


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_tree_view_gives_the_handed_over_trees_guides(form, device):
    """one sphere-only world per form of exact re-treeing, each in a fresh child process under its own time limit: the guides are those
    of the same world created with VK_SCENE_REFERENCE_TREE, bit for bit"""
    scene, seed, env, debug, tree, in_lds = FORMS[form]
    code = _FORM_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), debug=debug, scene=scene, seed=seed, w=FORM_W, tree=tree,
                              in_lds=in_lds)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FORM OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_call_shapes_are_bit_identical(device):
    import torch
    hs = HostScene("cornell_box", 1)
    cam = hs.next_camera()
    p = hs.params(40, 4, 50, seed=9, height=28)
    ds = DeviceScene(hs.desc)
    try:
        full, st = ds.render_guides(cam, p, first_sample=5)
        assert st.kernel_launches == 1 and st.samples == 40 * 28 * 4
        bufs = {ch: torch.zeros(v.shape, dtype=torch.float32, device="cuda:0") for ch, v in full.items()}
        ds.render_guides_device(cam, p, 5, None, *[bufs[ch].data_ptr() for ch in guides_ref.CHANNELS])
        torch.cuda.synchronize()
        for ch in full:
            np.testing.assert_array_equal(bufs[ch].cpu().numpy().view(np.uint32), full[ch].view(np.uint32), err_msg=ch)
        for ch in full:
            alone, _ = ds.render_guides(cam, p, first_sample=5, want=(ch,))
            np.testing.assert_array_equal(alone[ch].view(np.uint32), full[ch].view(np.uint32), err_msg=ch)
        # a tile partition of 3: a NaN sentinel outside, the union is the whole frame
        union = {ch: np.full_like(v, np.nan) for ch, v in full.items()}
        tile_of = (np.arange(28)[:, None] // 8) * 5 + (np.arange(40)[None, :] // 8)
        for rank in range(3):
            q = hs.params(40, 4, 50, seed=9, height=28, tile_rank=rank, tile_world=3)
            part, _ = ds.render_guides(cam, q, first_sample=5, out={ch: np.full_like(v, np.nan) for ch, v in full.items()})
            mine = tile_of % 3 == rank
            for ch in full:
                assert np.isnan(part[ch][~mine]).all(), ch
                union[ch][mine] = part[ch][mine]
        bits_equal(union, full, guides_ref.CHANNELS)
    finally:
        ds.close()
        hs.close()


def test_render_and_progress_are_not_disturbed(device):
    hs = HostScene("random_spheres_iow", 1)
    cam = hs.next_camera()
    p = hs.params(64, 16, 50, seed=4, height=48)
    ds = DeviceScene(hs.desc)
    try:
        launches = lambda: [bytes(x) for x in ffi.last_launches(ds._lib, ds._h)]
        a, _ = ds.render(cam, p)
        la = launches()
        g1, _ = ds.render_guides(cam, hs.params(64, 4, 50, seed=4, height=48))
        assert launches() == la
        b, _ = ds.render(cam, p)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        with ds.progress(cam, p) as pr:
            pr.step(6)
            g2, _ = ds.render_guides(cam, hs.params(64, 4, 50, seed=4, height=48))
            img, _ = pr.step(10)
        np.testing.assert_array_equal(img.view(np.uint32), a.view(np.uint32))
        bits_equal(g1, g2, guides_ref.CHANNELS)
    finally:
        ds.close()
        hs.close()


# ---------------------------------------------------------------- what the guides buy the denoiser
def quality_frame(seed=5, truth_seed=77):
    """tools/guides_report.py's InOneWeekend frame (tools/denoise_report.py's: 256x144, 16 spp in 4 windows and its standard error,
    reference vk_render at 8192 spp), denoised once from vk_render_aov's guides and once from vk_render_guides' at the defaults"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import guides_report
    hs = HostScene("random_spheres_iow", 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        return guides_report.quality_frame(ds, hs, cam, seed, truth_seed)
    finally:
        ds.close()
        hs.close()


# Measured on the MI355X (tools/guides_report.py --part quality).  Seed set (5, 77), the frame of section 6: relative
# MSE over the delta pixels (23.5 % of the frame) 0.012122 with first-hit guides, 0.010119 with the specular guides, r = 0.8348; over the
# frame 0.007999 -> 0.007583, ratio 0.9479.  The five seed sets give r = 0.8348, 1.0232, 0.8369, 0.8292, 0.7989 and whole-frame ratios
# from 0.9453 to 1.0180: a spread of 0.0726.
R_DELTA = 0.8348
FRAME_SPREAD = 0.0726


def test_guides_help_the_denoiser_where_the_frame_is_specular(device):
    """new guides over old, relative MSE of the denoised frame over the delta pixels (bounces >= 0.5): at most 1 - (1 - r) / 2 for the
    measured r, and below 1; over the whole frame the ratio may exceed 1 by no more than the spread five seed sets show."""
    q = quality_frame()
    print("\n   quality:", {k: round(v, 6) for k, v in q.items()})
    print("   ratio over delta pixels %.4f, over the frame %.4f" % (q["new_delta"] / q["old_delta"], q["new"] / q["old"]))
    r = q["new_delta"] / q["old_delta"]
    assert r <= 1.0 - (1.0 - R_DELTA) / 2.0 and r < 1.0, r
    assert q["new"] / q["old"] <= 1.0 + FRAME_SPREAD


def test_cli_guide_bounces(device, tmp_path):
    """vecchio_cli's trailing guide_bounces argument: 0 is absent, byte for byte in every file; a non-zero value adds the guide files,
    which are vk_render_guides' buffers, and denoises from them (vk_denoise of the same colour and error with those guides)"""
    from test_gpu_aov import _read_pfm
    from vecchio_amd import build
    cli = build.build_cli()
    base = ["random_spheres_iow", "64", "16", "10", "1", "1", "4", "4", "1", "0"]
    dirs = {}
    for key, extra in (("absent", []), ("zero", ["0"]), ("four", ["4"])):
        dirs[key] = tmp_path / key
        dirs[key].mkdir()
        subprocess.run([cli] + base + extra, cwd=dirs[key], check=True, timeout=300, capture_output=True)
    names = sorted(f.name for f in dirs["absent"].iterdir())
    assert sorted(f.name for f in dirs["zero"].iterdir()) == names
    for n in names:
        assert (dirs["absent"] / n).read_bytes() == (dirs["zero"] / n).read_bytes(), n
    guide_files = ["output_0000_guide_%s.pfm" % ch for ch in ("albedo", "normal", "depth", "bounces")]
    assert sorted(f.name for f in dirs["four"].iterdir()) == sorted(names + guide_files)
    for n in names:
        same = (dirs["absent"] / n).read_bytes() == (dirs["four"] / n).read_bytes()
        assert same == ("denoised" not in n), n
    hs = HostScene("random_spheres_iow", 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    try:
        got, _ = ds.render_guides(cam, hs.params(64, 4, 10, seed=2), guide=ds.guide_params(max_bounces=4))
        for ch in ("albedo", "normal", "depth", "bounces"):
            np.testing.assert_array_equal(_read_pfm(dirs["four"] / f"output_0000_guide_{ch}.pfm").view(np.uint32), got[ch].view(np.uint32),
                                          err_msg=ch)
        assert got["bounces"].max() >= 1
    finally:
        ds.close()
        hs.close()


def test_cli_temporal_from_the_guides(device, tmp_path):
    """vecchio_cli with temporal = 1 and denoise = 1 over three frames of an orbit: with guide_bounces = 4 the accumulator and the
    denoiser take the guides.  Frame 0 has no history; from frame 1 on the guides decide which taps are consistent, the accumulated
    images differ from those under first-hit guides, and most of the frame still finds history."""
    import re
    from test_gpu_aov import _read_pfm
    from vecchio_amd import build
    cli = build.build_cli()
    base = ["random_spheres_demo", "96", "8", "10", "3", "1", "2", "8", "1", "1"]
    outs = {}
    for key, extra in (("first_hit", ["0"]), ("guides", ["4"])):
        d = tmp_path / key
        d.mkdir()
        r = subprocess.run([cli] + base + extra, cwd=d, timeout=300, capture_output=True, text=True,
                           env=dict(os.environ, VECCHIO_ASSETS=os.path.join(ROOT, "tests", "golden", "assets")))
        assert r.returncode == 0, r.stderr[-2000:]
        shares = [float(x) for x in re.findall(r"accumulated: ([0-9.]+) % of the pixels with history", r.stderr)]
        assert len(shares) == 3 and shares[0] == 0.0, r.stderr[-2000:]
        outs[key] = (d, shares)
        print("\n   %s: pixels with history per frame %s" % (key, shares))
    a, b = outs["first_hit"][0], outs["guides"][0]
    assert (a / "output_0002_temporal.pfm").read_bytes() != (b / "output_0002_temporal.pfm").read_bytes()
    for n in ("output_0002.ppm", "output_0002_albedo.pfm"):
        assert (a / n).read_bytes() == (b / n).read_bytes(), n
    assert np.isfinite(_read_pfm(b / "output_0002_temporal.pfm")).all() and np.isfinite(_read_pfm(b / "output_0002_denoised.pfm")).all()
    assert (b / "output_0002_guide_bounces.pfm").exists() and _read_pfm(b / "output_0002_guide_bounces.pfm").max() >= 1
    assert min(outs["guides"][1][1:]) > 50.0
