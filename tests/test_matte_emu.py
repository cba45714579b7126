"""ID mattes on the CPU: vk_matte.h matte_sample, matte_insert and matte_sort (through tests/emu, on the tree view and with the kernel
instance vk_api.hip chooses) against the CPU oracle, per sample and bit for bit, on every scene tests/test_aov_emu.py uses:
  MATERIAL ids  = oracle_first_hits' `hit ? material : BACKGROUND`, every sample, media included;
  OBJECT ids    = emu_rays' `object` on the oracle's primary rays, in the media-free scenes (a medium met by a ray query draws from
                  another stream); in media scenes the id's kind is VK_KIND_MEDIUM exactly where the oracle says `medium`, and that
                  vk_medium's material is the oracle's;
  tables        = tests/matte_ref.py applied to those per-sample ids."""
import itertools

import numpy as np
import pytest

import emu_matte_ffi
import emu_queries_ffi
import matte_ref
import special_scenes
from test_aov_emu import EXTRA, SAMPLES, SIZE, special
from test_emu_parity import BUILDER_SCENES
from vecchio_amd import ffi
from vecchio_amd.scene import make_rays

BG = ffi.VK_MATTE_BACKGROUND


def check_scene(oracle, desc, cam, p, samples=SAMPLES):
    first, n = samples[0], len(samples)
    fh = oracle.first_hits(desc, cam, p, first, n)
    want_mat = np.where(fh["hit"] == 1, fh["material"], np.uint32(BG)).astype(np.uint32)
    mat, features = emu_matte_ffi.matte_samples(desc, cam, p, first, n, ffi.VK_MATTE_MATERIAL)
    np.testing.assert_array_equal(mat, want_mat)
    obj, _ = emu_matte_ffi.matte_samples(desc, cam, p, first, n, ffi.VK_MATTE_OBJECT)
    np.testing.assert_array_equal(obj == BG, fh["hit"] == 0)
    hit = fh["hit"] == 1
    assert not (obj[hit] & ffi.VK_REF_FLIP).any()
    kind = obj >> 28
    if desc.contents.n_media == 0:
        flat = fh.reshape(-1)
        hits, _ = emu_queries_ffi.trace_rays(desc, make_rays(flat["origin"], flat["direction"], flat["time"]))
        np.testing.assert_array_equal(hits["hit"], flat["hit"])
        np.testing.assert_array_equal(obj.reshape(-1)[flat["hit"] == 1], hits["object"][flat["hit"] == 1])
        assert not (kind[hit] == ffi.VK_KIND_MEDIUM).any()
    else:
        med = fh["medium"] == 1
        np.testing.assert_array_equal(hit & (kind == ffi.VK_KIND_MEDIUM), med)
        idx = obj[med] & ffi.VK_REF_INDEX_MASK
        assert (idx < desc.contents.n_media).all()
        media_mat = np.array([desc.contents.media[i].material for i in range(desc.contents.n_media)], np.uint32)
        np.testing.assert_array_equal(media_mat[idx], fh["material"][med])
        surface = hit & ~med
        assert np.isin(kind[surface], (ffi.VK_KIND_SPHERE, ffi.VK_KIND_MOVING_SPHERE, ffi.VK_KIND_RECT)).all()
    # the window's table is the rule of the header applied to the per-sample ids
    for k, ids_of, ranks in ((ffi.VK_MATTE_MATERIAL, mat, 2), (ffi.VK_MATTE_OBJECT, obj, 3), (ffi.VK_MATTE_MATERIAL, mat, 8)):
        got = emu_matte_ffi.matte_window(desc, cam, p, first, n, k, ranks)
        want = matte_ref.table(ids_of, ranks)
        for g, w, what in zip(got, want, ("ids", "counts", "overflow")):
            np.testing.assert_array_equal(g, w, err_msg=f"{what}, kind {k}, ranks {ranks}")
        assert (got[1].sum(-1) + got[2] == n).all()
    return fh, mat, obj, features


@pytest.mark.parametrize("name", BUILDER_SCENES)
def test_builder_scene_per_sample(name, oracle, emu, host_scenes):
    hs, cam = host_scenes(name)
    p = hs.params(SIZE, 2, 50, seed=7, height=SIZE)
    fh, _, _, features = check_scene(oracle, hs.desc, cam, p)
    assert (features == 0) == name.startswith("random_spheres_iow")
    if hs.desc.contents.n_media > 0:
        assert (fh["medium"] == 1).any() and ((fh["hit"] == 1) & (fh["medium"] == 0)).any()


@pytest.mark.parametrize("name", sorted(special_scenes.ALL))
def test_special_scene_per_sample(name, oracle, emu, built):
    d, desc, cam, p = special(name)
    check_scene(oracle, desc, cam, p)


@pytest.mark.parametrize("name", sorted(EXTRA))
def test_extra_media_scene_per_sample(name, oracle, emu, built):
    d, desc, cam, p = EXTRA[name]()
    fh, _, _, _ = check_scene(oracle, desc, cam, p, samples=(0, 1, 2, 3))
    assert (fh["medium"] == 1).any() and ((fh["hit"] == 1) & (fh["medium"] == 0)).any()


def test_a_window_that_does_not_start_at_zero_and_a_partition(oracle, emu, host_scenes):
    hs, cam = host_scenes("cornell_box")
    p = hs.params(21, 1, 50, seed=7, height=13)
    fh = oracle.first_hits(hs.desc, cam, p, 5, 7)
    want = np.where(fh["hit"] == 1, fh["material"], np.uint32(BG)).astype(np.uint32)
    whole = emu_matte_ffi.matte_window(hs.desc, cam, p, 5, 7, ffi.VK_MATTE_MATERIAL, 3)
    for g, w in zip(whole, matte_ref.table(want, 3)):
        np.testing.assert_array_equal(g, w)
    p.tile_world, p.tile_rank = 3, 1
    part = emu_matte_ffi.matte_window(hs.desc, cam, p, 5, 7, ffi.VK_MATTE_MATERIAL, 3)
    # tile = (y / 8) * tiles_x + x / 8 with tiles_x = 3
    mine =(np.arange(13)[:, None] // 8 * 3 + np.arange(21)[None, :] // 8) % 3 == 1
    assert mine.any() and not mine.all()
    for g, w in zip(part, whole):
        np.testing.assert_array_equal(g[mine], w[mine])
        assert (g[~mine] == 0xDEADBEEF).all()


@pytest.mark.parametrize("ranks", [1, 2, 3, 5, 8])
def test_insert_and_sort_against_the_reference(ranks, built):
    """the table's compare-and-select code alone: random id sequences with few and with many distinct ids (ties in count, ids on both
    sides of 2^31, BACKGROUND and 0 among them), and every 0/1 pattern of eight counts through the sorting network"""
    rng = np.random.default_rng(100 + ranks)
    pool = np.array([0, 1, 2, 7, 0x20000003, 0x40000001, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, BG, 5], np.uint32)
    for trial in range(300):
        n = int(rng.integers(1, 40))
        seq = rng.choice(pool[:int(rng.integers(1, len(pool) + 1))], size=n).astype(np.uint32)
        ids, counts, over = emu_matte_ffi.table(seq, ranks)
        w_ids, w_counts, w_over = matte_ref.table(seq[None, :], ranks)
        np.testing.assert_array_equal(ids, w_ids[0])
        np.testing.assert_array_equal(counts, w_counts[0])
        assert over == w_over[0] and counts.sum() + over == n
    if ranks == 8:
        # counts 1 or 2 in every arrangement over eight slots taken in the order of their (descending) ids: the network sorts them all
        for bits in itertools.product((1, 2), repeat=8):
            seq = np.concatenate([np.full(c, 100 - i, np.uint32) for i, c in enumerate(bits)])
            ids, counts, over = emu_matte_ffi.table(seq, 8)
            w = matte_ref.table(seq[None, :], 8)
            np.testing.assert_array_equal(ids, w[0][0])
            np.testing.assert_array_equal(counts, w[1][0])
            assert over == 0
