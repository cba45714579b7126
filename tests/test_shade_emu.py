"""Shade queries on the CPU: vk_trace.h shade_hit (through tests/emu/emu_shade.cpp) in the loop of vk_shade_hits' contract around the rays
emulator, against the radiance emulator (vk_trace.h radiance_sample, which the existing suite ties to the oracle): in every scene
without a ConstantMedium the loop's radiance and final stream counter equal the radiance query's sample bit for bit, for both
integrators and two depth limits.  The two sides are the two forms of ONE body, vk_trace.h shade_core: shade_hit runs its record form
(the hit as the caller's record), radiance_sample its walk form (the hit as the walk left it in the lane).  With media the loop runs to its end on valid records.  Bad hits are refused per item.
tests/test_gpu_shade.py runs the same scenes and rays on the device."""
import numpy as np
import pytest

import shade_ref as S
from vecchio_amd import ffi
from vecchio_amd.scene import make_path_states

f32 = np.float32


@pytest.fixture(scope="session")
def emu_shade(built):
    import emu_shade_ffi
    emu_shade_ffi.load()
    return emu_shade_ffi


@pytest.fixture(scope="session")
def emu_queries(built):
    import emu_queries_ffi
    emu_queries_ffi.load()
    return emu_queries_ffi


def test_the_media_free_scenes_hold_every_kind(host_scenes):
    plain, media = S.split_by_media(host_scenes)
    assert len(plain) >= 10 and len(media) >= 2, (plain, media)
    mats, texs, lights = set(), set(), set()
    for kind, name in plain:
        m, t, l = S.census(S.scene(kind, name, host_scenes)[0])
        mats |= m; texs |= t; lights |= l
    assert {ffi.VK_MAT_LAMBERTIAN, ffi.VK_MAT_METAL, ffi.VK_MAT_DIELECTRIC, ffi.VK_MAT_DIFFUSE_LIGHT, ffi.VK_MAT_SPEC_DIFFUSE} <= mats, mats
    assert {ffi.VK_TEX_SOLID, ffi.VK_TEX_CHECKER, ffi.VK_TEX_IMAGE, ffi.VK_TEX_NOISE} <= texs, texs
    assert {ffi.VK_KIND_RECT, ffi.VK_KIND_SPHERE} <= lights, lights


@pytest.mark.parametrize("kind,name", S.ALL_SCENES, ids=[f"{k}-{n}" for k, n in S.ALL_SCENES])
def test_loop_on_scene(kind, name, emu_shade, emu_queries, host_scenes):
    desc, cam, p = S.scene(kind, name, host_scenes)
    rays = S.rays_of(cam)
    integrators = S.integrators(desc)
    assert integrators
    lobes = set()
    for integrator in integrators:
        for depth in S.DEPTHS:
            what = f"{kind} {name}, integrator {integrator}, max_depth {depth}"
            got, bounces = emu_shade.wavefront(desc, rays, S.SEED, S.FIRST, 0, **S.shade_kwargs(p, integrator, depth))
            assert 1 <= len(bounces) <= depth, what                       # (the hit at depth max_depth ends the path)
            for b in bounces:
                out, hits = b["out"], b["hits"]
                assert np.isin(out["status"], S.STATUSES[:3]).all(), what
                go = out["status"] == ffi.VK_SHADE_SCATTERED
                np.testing.assert_array_equal(out["next"]["origin"][go].view(np.uint32), hits["p"][go].view(np.uint32))
                assert np.isposinf(out["next"]["tmax"][go]).all() and not out["next"][~go].view(np.uint32).any(), what
                assert (out["status"][hits["hit"] == 0] == ffi.VK_SHADE_MISS).all() and (out["lobe"][hits["hit"] == 0] == 0xFFFFFFFF).all()
                assert not out["_pad"].any()
                shaded = hits["hit"] == 1
                assert (out["lobe"][shaded & (hits["medium"] == 1)] == ffi.VK_MAT_ISOTROPIC).all(), what
                lobes |= set(out["lobe"][shaded].tolist())
            if desc.contents.n_media:
                continue
            want, _ = emu_queries.radiance_samples(desc, rays, **S.radiance_kwargs(p, integrator, depth))
            S.assert_samples_equal(got, want[:, 0], what)
            assert got[:, 3].view(np.uint32).max() > 0, what            # something was drawn
    print(f"\n   {kind} {name}: media {desc.contents.n_media}, integrators {integrators}, lobes sampled {sorted(lobes)}")
    assert lobes <= set(range(6))


def test_a_later_sample_and_a_cut_batch(emu_shade, emu_queries, host_scenes):
    """sample 2 of the radiance query is the loop started with sample = 2; a batch cut in two with matching first_index is the batch"""
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    rays = S.rays_of(cam)
    kw = S.shade_kwargs(p, p.integrator, 8)
    want, _ = emu_queries.radiance_samples(desc, rays, **S.radiance_kwargs(p, p.integrator, 8, samples_per_ray=3))
    got, _ = emu_shade.wavefront(desc, rays, S.SEED, S.FIRST, 2, **kw)
    S.assert_samples_equal(got, want[:, 2], "sample 2")
    cut = len(rays) // 3
    a, _ = emu_shade.wavefront(desc, rays[:cut], S.SEED, S.FIRST, 2, **kw)
    b, _ = emu_shade.wavefront(desc, rays[cut:], S.SEED, S.FIRST + cut, 2, **kw)
    np.testing.assert_array_equal(np.concatenate([a, b]).view(np.uint32), got.view(np.uint32))


def bad_hit_batch(desc, cam, trace):
    """(rays, hits, states, bad, index of the items made bad): a traced batch in which two hits are spoiled — hit = 2, and material =
    the description's material count — with mid-path states"""
    rays = S.rays_of(cam)
    hits = trace(rays)
    states = make_path_states(len(rays), S.SEED, S.FIRST, 1)
    states["thr"] = f32([0.5, 0.25, 0.125]); states["acc"] = f32([1.0, 2.0, 3.0]); states["depth"] = 3; states["counter"] = 11
    hit = np.flatnonzero(hits["hit"] == 1)
    assert len(hit) > 8
    i, j = int(hit[3]), int(hit[len(hit) // 2])
    bad = hits.copy()
    bad["hit"][i] = 2
    bad["material"][j] = desc.contents.n_materials
    return rays, hits, states, bad, (i, j)


def check_bad_hits(good, spoiled, states, where, what=""):
    """the two spoiled items are BAD_HIT with the state copied through; every other item is what it was"""
    for k in where:
        assert spoiled["status"][k] == ffi.VK_SHADE_BAD_HIT and spoiled["lobe"][k] == 0xFFFFFFFF, (what, k)
        assert spoiled["state"][k].tobytes() == states[k].tobytes(), (what, k)
        assert not spoiled["next"][k:k + 1].view(np.uint32).any() and not spoiled["_pad"][k].any(), (what, k)
        assert good["status"][k] in (ffi.VK_SHADE_SCATTERED, ffi.VK_SHADE_ENDED), (what, k)
    keep = np.ones(len(good), bool)
    keep[list(where)] = False
    S.assert_shaded_equal(spoiled[keep], good[keep], what)


@pytest.mark.parametrize("kind,name", [("builder", "cornell_box"), ("builder", "final_scene")])
def test_bad_hits_are_refused_per_item(kind, name, emu_shade, emu_queries, host_scenes):
    desc, cam, p = S.scene(kind, name, host_scenes)
    rays, hits, states, bad, where = bad_hit_batch(desc, cam, lambda r: emu_queries.trace_rays(desc, r, S.SEED, S.FIRST)[0])
    kw = S.shade_kwargs(p, p.integrator, 50)
    good = emu_shade.shade_hits(desc, rays, hits, states, **kw)
    spoiled = emu_shade.shade_hits(desc, rays, bad, states, **kw)
    check_bad_hits(good, spoiled, states, where, f"{kind} {name}")
    # a material index far outside the table, and hit = 0xFFFFFFFF
    bad["material"][where[1]] = 0xFFFFFFFF
    bad["hit"][where[0]] = 0xFFFFFFFF
    check_bad_hits(good, emu_shade.shade_hits(desc, rays, bad, states, **kw), states, where, f"{kind} {name}, extreme")
    # a miss does not read its material field
    miss = hits.copy()
    k = int(np.flatnonzero(hits["hit"] == 0)[0]) if (hits["hit"] == 0).any() else None
    if k is not None:
        miss["material"][k] = 0xFFFFFFFF
        out = emu_shade.shade_hits(desc, rays, miss, states, **kw)
        assert out["status"][k] == ffi.VK_SHADE_MISS
        S.assert_shaded_equal(out, good, "a miss with a wild material index")
