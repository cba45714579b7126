"""ID mattes (vk_render_mattes) on the MI355X, through the C ABI.  Every comparison is bit for bit: the per-sample ids of the debug hook
against the CPU oracle (MATERIAL) and against vk_trace_rays on the oracle's rays (OBJECT, media-free scenes); the tables against
tests/matte_ref.py applied to the hook's ids; windows merged by vk_matte_merge against the one call; tile partitions; the coverage of
vk_render_aov recovered from the background's count; every tree view a scene can take; and what a call must leave alone.

Frames of 21 x 13 pixels (partial tiles on both axes), seed 7: cornell_box (the everything instance), random_spheres_iow (the sphere-only
instance) and final_scene (media)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aov_ref
import matte_ref
from vecchio_amd import DeviceScene, HostScene, ffi
from vecchio_amd.scene import make_rays, matte_mask, matte_merge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SEED = 21, 13, 7
SCENES = ("cornell_box", "random_spheres_iow", "final_scene")
KINDS = (ffi.VK_MATTE_OBJECT, ffi.VK_MATTE_MATERIAL)
BG = ffi.VK_MATTE_BACKGROUND
N_HOOK = 69                      # samples 0 .. 68: every window below lies inside


class Shared:
    """a scene on the device and the hook's ids of samples 0 .. N_HOOK - 1 under both kinds, computed once and never written to"""

    def __init__(self, name):
        self.name = name
        self.hs = HostScene(name, 1)
        self.cam = self.hs.next_camera()
        self.desc = self.hs.desc
        self.ds = DeviceScene(self.desc)
        self.ids = {k: self.ds.debug_matte_samples(self.cam, self.params(N_HOOK), 0, k) for k in KINDS}
        for a in self.ids.values():
            a.flags.writeable = False

    def params(self, spp, **kw):
        return self.hs.params(W, spp, 50, seed=SEED, height=H, **kw)

    def close(self):
        self.ds.close()
        self.hs.close()


@pytest.fixture(scope="module")
def scenes(device):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Shared(name)
        return made[name]

    yield get
    for s in made.values():
        s.close()


def equal(got, want, where=None, what=""):
    for g, w, ch in zip(got, want, ("ids", "counts", "overflow")):
        if g is None or w is None:
            continue
        np.testing.assert_array_equal(g if where is None else g[where], w if where is None else w[where], err_msg=f"{what} {ch}")


# ---------------------------------------------------------------- 1. the ids of single samples
@pytest.mark.parametrize("name", SCENES)
def test_sample_ids_against_the_oracle_and_the_ray_queries(name, scenes, oracle):
    s = scenes(name)
    fh = oracle.first_hits(s.desc, s.cam, s.params(4), 0, 4)
    mat = s.ds.debug_matte_samples(s.cam, s.params(4), 0, ffi.VK_MATTE_MATERIAL)
    obj = s.ds.debug_matte_samples(s.cam, s.params(4), 0, ffi.VK_MATTE_OBJECT)
    hit = fh["hit"] == 1
    np.testing.assert_array_equal(mat, np.where(hit, fh["material"], np.uint32(BG)).astype(np.uint32))
    np.testing.assert_array_equal(obj == BG, ~hit)
    # the hook's window is the call's: the shared 69-sample run starts with these four
    np.testing.assert_array_equal(s.ids[ffi.VK_MATTE_MATERIAL][..., :4], mat)
    np.testing.assert_array_equal(s.ids[ffi.VK_MATTE_OBJECT][..., :4], obj)
    kind = obj >> 28
    assert not (obj[hit] & ffi.VK_REF_FLIP).any()
    if s.desc.contents.n_media == 0:
        flat = fh.reshape(-1)
        hits = s.ds.trace_rays(make_rays(flat["origin"], flat["direction"], flat["time"]))
        np.testing.assert_array_equal(hits["hit"], flat["hit"])
        np.testing.assert_array_equal(obj.reshape(-1), np.where(hits["hit"] == 1, hits["object"], np.uint32(BG)).astype(np.uint32))
        assert hit.any()
    else:
        med = fh["medium"] == 1
        assert med.any() and (hit & ~med).any()
        np.testing.assert_array_equal(hit & (kind == ffi.VK_KIND_MEDIUM), med)
        idx = obj[med] & ffi.VK_REF_INDEX_MASK
        assert (idx < s.desc.contents.n_media).all()
        media_mat = np.array([s.desc.contents.media[i].material for i in range(s.desc.contents.n_media)], np.uint32)
        np.testing.assert_array_equal(media_mat[idx], fh["material"][med])
    assert (s.ds.info().features == 0) == (name == "random_spheres_iow")


# ---------------------------------------------------------------- 2. the tables
@pytest.mark.parametrize("name", SCENES)
def test_tables_against_the_reference(name, scenes):
    s = scenes(name)
    seen_overflow = seen_clean = 0
    for kind in KINDS:
        for first in (0, 5):
            for spp in (1, 7, 64):
                window = s.ids[kind][..., first:first + spp]
                for ranks in (1, 2, 3, 8):
                    want = matte_ref.table(window, ranks)
                    got = s.ds.render_mattes(s.cam, s.params(spp), first, kind, ranks)
                    equal(got, want, what=f"kind {kind} first {first} spp {spp} ranks {ranks}")
                    assert (got[1].sum(-1, dtype=np.uint64) + got[2] == spp).all()
                    bare = s.ds.render_mattes(s.cam, s.params(spp), first, kind, ranks, overflow=False)
                    assert bare[2] is None
                    equal(bare[:2], want[:2], what="without overflow")
                    seen_overflow += int((got[2] != 0).sum())
                    seen_clean += int((got[2] == 0).sum())
    assert seen_overflow > 0 and seen_clean > 0
    ids, counts, over = s.ds.render_mattes(s.cam, s.params(64), 0, ffi.VK_MATTE_MATERIAL, 8)
    if name == "random_spheres_iow":
        assert int((over != 0).sum()) == 3           # up to 10 materials in a pixel
    if name == "cornell_box":
        assert not s.ds.render_mattes(s.cam, s.params(64), 0, ffi.VK_MATTE_MATERIAL, 3)[2].any()       # at most 3
    # the mask of everything the table kept
    everything = np.unique(ids[counts != 0])
    np.testing.assert_array_equal(matte_mask(ids, counts, 64, everything), (64 - over).astype(np.float32) / np.float32(64))


# ---------------------------------------------------------------- 3. windows merged
@pytest.mark.parametrize("name", SCENES)
def test_windows_merge_into_the_one_call(name, scenes):
    s = scenes(name)
    lib = s.ds._lib
    seen_overflow = seen_clean = 0
    for kind, ranks in ((ffi.VK_MATTE_MATERIAL, 8), (ffi.VK_MATTE_OBJECT, 3), (ffi.VK_MATTE_MATERIAL, 2)):
        whole = s.ds.render_mattes(s.cam, s.params(64), 0, kind, ranks)
        parts = [s.ds.render_mattes(s.cam, s.params(16), 16 * w, kind, ranks) for w in range(4)]
        clean = whole[2] == 0
        for order in ((0, 1, 2, 3), (2, 0, 3, 1)):
            a = tuple(x.copy() for x in parts[order[0]])
            for w in order[1:]:
                matte_merge(*a, *parts[w], lib=lib)
            equal(a, whole, clean, what=f"kind {kind} ranks {ranks} order {order}")
            np.testing.assert_array_equal(a[2] == 0, clean)
            assert (a[1].sum(-1, dtype=np.uint64) + a[2] == 64).all()
        seen_overflow += int((~clean).sum())
        seen_clean += int(clean.sum())
    assert seen_overflow > 0 and seen_clean > 0


# ---------------------------------------------------------------- 4. tile partitions
@pytest.mark.parametrize("name", ("cornell_box", "random_spheres_iow"))
def test_partitions_leave_the_rest_untouched(name, scenes):
    s = scenes(name)
    tile_of = (np.arange(H)[:, None] // 8) * 3 + (np.arange(W)[None, :] // 8)
    for kind, ranks in ((ffi.VK_MATTE_OBJECT, 4), (ffi.VK_MATTE_MATERIAL, 3)):
        whole = s.ds.render_mattes(s.cam, s.params(7), 5, kind, ranks)
        union = tuple(np.full_like(x, 0xDEADBEEF) for x in whole)
        samples = 0
        for rank in range(3):
            out = tuple(np.full_like(x, 0xDEADBEEF) for x in whole)
            *part, st = s.ds.render_mattes(s.cam, s.params(7, tile_rank=rank, tile_world=3), 5, kind, ranks, out=out, return_stats=True)
            mine = tile_of % 3 == rank
            assert mine.any()
            assert st.samples == int(mine.sum()) * 7 and st.kernel_launches == 1 and st.kernel_ms > 0
            samples += st.samples
            for u, g in zip(union, part):
                assert (g[~mine] == 0xDEADBEEF).all()
                u[mine] = g[mine]
            hook = s.ds.debug_matte_samples(s.cam, s.params(7, tile_rank=rank, tile_world=3), 5, kind, out=np.full((H, W, 7), 0xDEADBEEF, np.uint32))
            assert (hook[~mine] == 0xDEADBEEF).all()
            np.testing.assert_array_equal(hook[mine], s.ids[kind][..., 5:12][mine])
        equal(union, whole)
        assert samples == W * H * 7


# ---------------------------------------------------------------- 5. the anchor: vk_render_aov's coverage
@pytest.mark.parametrize("name", ("cornell_box", "random_spheres_iow"))
def test_background_count_gives_the_first_hit_coverage(name, scenes, oracle):
    s = scenes(name)
    n = 64
    ref = aov_ref.ref_a(oracle, s.desc, s.cam, s.params(n), list(range(n)))
    assert not ref["dropped"].any()                    # the frame drops no sample: no pixel is left out for that reason
    cov = s.ds.render_aov(s.cam, s.params(n), want=("coverage",))[0]["coverage"]
    compared = 0
    for kind in KINDS:
        ids, counts, over = s.ds.render_mattes(s.cam, s.params(n), 0, kind, 8)
        bg = np.where((ids == BG) & (counts != 0), counts, 0).sum(-1)
        got = (n - bg).astype(np.float32) / np.float32(n)
        clean = over == 0
        np.testing.assert_array_equal(got[clean].view(np.uint32), cov[clean].view(np.uint32))
        np.testing.assert_array_equal(matte_mask(ids, counts, n, [BG])[clean], (np.float32(1) - cov)[clean])   # k / 64 is exact
        compared += int(clean.sum())
    assert compared > W * H


# ---------------------------------------------------------------- 6. every tree view
FORMS = {
    "grid_lds": ("random_spheres_iow", 1, {}, False, "VK_TREE_REBUILT_GRID", True),
    "near_lds": ("random_spheres_iow", 3, {"VK_NO_GRID": "1"}, False, "VK_TREE_REBUILT_NEAR", True),
    "near_global": ("stress_spheres:30", 1, {}, False, "VK_TREE_REBUILT_NEAR", False),
    "unit_lds": ("random_spheres_iow", 1, {"VK_NEAR_FIRST": "0", "VK_NO_GRID": "1"}, True, "VK_TREE_REBUILT_PROVEN", True),
}

_FORM_CHILD = """
import sys
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
    p = hs.params(%(w)d, 8, 50, seed=%(pseed)d, height=%(h)d)
    got = [ds.render_mattes(cam, p, 3, kind, 4) for kind in (ffi.VK_MATTE_OBJECT, ffi.VK_MATTE_MATERIAL)]
    got.append((ds.debug_matte_samples(cam, p, 3, ffi.VK_MATTE_OBJECT),))
    again, _ = ds.render(cam, hs.params(128, 8, 50, seed=3))
    assert np.array_equal(img.view(np.uint32), again.view(np.uint32))
    res[flags] = (tree, in_lds, got)
    ds.close(); hs.close()
tree, in_lds, got = res[0]
rtree, _, rgot = res[ffi.VK_SCENE_REFERENCE_TREE]
assert tree == ffi.%(tree)s and in_lds == %(in_lds)r, (tree, in_lds)
assert rtree == ffi.VK_TREE_HANDED_OVER, rtree
for a, b in zip(got, rgot):
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
assert (got[0][1].sum(-1) + got[0][2] == 8).all() and (got[0][0] != ffi.VK_MATTE_BACKGROUND).any()
print("FORM OK", tree, in_lds)
"""


@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_tree_view_gives_the_handed_over_trees_tables(form, device):
    """one sphere-only world per form of exact re-treeing, each in a fresh child process (the switches are read at scene creation): the
    child asserts the form it runs and that tables and per-sample ids are those of the same world created with VK_SCENE_REFERENCE_TREE"""
    scene, seed, env, debug, tree, in_lds = FORMS[form]
    code = _FORM_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), debug=debug, scene=scene, seed=seed, w=W, h=H, pseed=SEED,
                              tree=tree, in_lds=in_lds)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FORM OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_fast_accel_walks_the_rebuilt_tree_to_the_same_ids(device, oracle):
    """under VK_SCENE_FAST_ACCEL the rebuilt tree is walked (ties as the reference breaks them): the oracle's materials, per sample"""
    hs = HostScene("random_spheres_iow", 1)
    hs.desc.contents.flags = ffi.VK_SCENE_FAST_ACCEL
    cam = hs.next_camera()
    p = hs.params(W, 4, 50, seed=SEED, height=H)
    ds = DeviceScene(hs.desc)
    try:
        fh = oracle.first_hits(hs.desc, cam, p, 0, 4)
        mat = ds.debug_matte_samples(cam, p, 0, ffi.VK_MATTE_MATERIAL)
        np.testing.assert_array_equal(mat, np.where(fh["hit"] == 1, fh["material"], np.uint32(BG)).astype(np.uint32))
    finally:
        ds.close()
        hs.close()


# ---------------------------------------------------------------- 7. what a call leaves alone, what it refuses, a multi-device scene
def test_nothing_else_is_disturbed(device):
    import torch
    hs = HostScene("random_spheres_iow", 1)
    cam = hs.next_camera()
    p = hs.params(64, 16, 50, seed=4, height=48)
    small = hs.params(W, 4, 50, seed=SEED, height=H)
    ds = DeviceScene(hs.desc)
    try:
        launches = lambda: [bytes(x) for x in ffi.last_launches(ds._lib, ds._h)]
        a, sa = ds.render(cam, p)
        la, ra, ms = launches(), ds.last_requeued_samples(), ds.last_kernel_ms()
        ds.render_mattes(cam, small, 0, ffi.VK_MATTE_OBJECT, 6)
        assert launches() == la and ds.last_requeued_samples() == ra and ds.last_kernel_ms() == ms
        b, sb = ds.render(cam, p)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        assert launches() == la and ds.last_requeued_samples() == ra and sb.clamped_samples == sa.clamped_samples
        # a progress handle interrupted by a matte call
        with ds.progress(cam, p) as pr:
            pr.step(6)
            ds.render_mattes(cam, small, 3, ffi.VK_MATTE_MATERIAL, 2)
            img, _ = pr.step(10)
        np.testing.assert_array_equal(img.view(np.uint32), a.view(np.uint32))
        # vk_render_aov's buffers, enqueued before a matte call and read after it
        full, _ = ds.render_aov(cam, small, first_sample=2)
        bufs = {ch: torch.zeros(v.shape, dtype=torch.float32, device="cuda:0") for ch, v in full.items()}
        ds.render_aov_device(cam, small, 2, bufs["albedo"].data_ptr(), bufs["normal"].data_ptr(), bufs["depth"].data_ptr(),
                             bufs["coverage"].data_ptr())
        t1 = ds.render_mattes(cam, small, 0, ffi.VK_MATTE_OBJECT, 8)
        torch.cuda.synchronize()
        for ch in full:
            np.testing.assert_array_equal(bufs[ch].cpu().numpy().view(np.uint32), full[ch].view(np.uint32), err_msg=ch)
        again, _ = ds.render_aov(cam, small, first_sample=2)
        for ch in full:
            np.testing.assert_array_equal(again[ch].view(np.uint32), full[ch].view(np.uint32), err_msg=ch)
        # ... and a ray query in between changes no table
        ds.trace_rays(make_rays([[0, 1, 5]], [[0, 0, -1]]))
        equal(ds.render_mattes(cam, small, 0, ffi.VK_MATTE_OBJECT, 8), t1)
        # a multi-device scene: on devices[0]
        multi = DeviceScene(hs.desc, devices=[0, 0])
        try:
            equal(multi.render_mattes(cam, small, 0, ffi.VK_MATTE_OBJECT, 8), t1)
        finally:
            multi.close()
    finally:
        ds.close()
        hs.close()


def test_refusals_leave_the_outputs_untouched(device):
    hs = HostScene("cornell_box", 1)
    cam = hs.next_camera()
    ds = DeviceScene(hs.desc)
    lib = ds._lib
    try:
        good = hs.params(16, 2, 50, height=16)
        ok = ffi.MatteParams(ffi.VK_MATTE_OBJECT, 6, 0, 0)
        ids, counts, over = (np.full(16 * 16 * 8, 7, np.uint32) for _ in range(3))
        I, N, O = (C.c_void_p(a.ctypes.data) for a in (ids, counts, over))
        cases = []
        q = hs.params(16, 2, 50, height=16); q.samples_per_pixel = 0; cases.append((q, 0, cam, ok))
        cases.append((good, 0xFFFFFFFF - 1, cam, ok))
        cases.append((hs.params(16, 2, 50, height=1), 0, cam, ok))
        cases.append((hs.params(1, 2, 50, height=16), 0, cam, ok))
        cases.append((hs.params(16, 2, 50, height=16, tile_rank=3, tile_world=3), 0, cam, ok))
        bad_cam = ffi.Camera(); C.pointer(bad_cam)[0] = cam; bad_cam.time1 = bad_cam.time0; cases.append((good, 0, bad_cam, ok))
        for mp in (ffi.MatteParams(2, 6, 0, 0), ffi.MatteParams(0, 0, 0, 0), ffi.MatteParams(0, 9, 0, 0), ffi.MatteParams(0, 6, 4, 0)):
            cases.append((good, 0, cam, mp))
        for q, first, c, mp in cases:
            st = lib.vk_render_mattes(ds._h, C.byref(c), C.byref(q), first, C.byref(mp), I, N, O, None)
            assert st == ffi.VK_ERR_BAD_ARG, (st, lib.vk_last_error())
        assert lib.vk_render_mattes(ds._h, C.byref(cam), C.byref(good), 0, None, I, N, O, None) == ffi.VK_ERR_BAD_ARG
        assert lib.vk_render_mattes(ds._h, C.byref(cam), C.byref(good), 0, C.byref(ok), None, N, O, None) == ffi.VK_ERR_BAD_ARG
        assert lib.vk_render_mattes(ds._h, C.byref(cam), C.byref(good), 0, C.byref(ok), I, None, O, None) == ffi.VK_ERR_BAD_ARG
        assert lib.vk_debug_matte_samples(ds._h, C.byref(cam), C.byref(good), 0, 2, I) == ffi.VK_ERR_BAD_ARG
        assert lib.vk_debug_matte_samples(ds._h, C.byref(cam), C.byref(good), 0, 0, None) == ffi.VK_ERR_BAD_ARG
        assert (ids == 7).all() and (counts == 7).all() and (over == 7).all()
        # output_format, max_depth, integrator and the background are not read
        base = ds.render_mattes(cam, good, 0, ffi.VK_MATTE_MATERIAL, 4)
        other = hs.params(16, 2, 3, height=16, output_format=ffi.VK_OUTPUT_RGB8)
        other.integrator = ffi.VK_INTEGRATOR_SCATTER
        other.background = ffi.VK_BACKGROUND_SKY
        equal(ds.render_mattes(cam, other, 0, ffi.VK_MATTE_MATERIAL, 4), base)
    finally:
        ds.close()
        hs.close()
