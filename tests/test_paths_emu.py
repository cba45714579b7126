"""Path batches on the CPU: the loop of vk_paths_step — vk_trace.h trace_path (through tests/emu/emu_paths.cpp), the shade emulator and
the numpy compaction of tests/paths_ref.py — against the radiance emulator (vk_trace.h radiance_sample) in EVERY scene of the shade
tests' set, ConstantMedium included: radiance and final stream counter bit for bit, for both integrators and two depth limits.  The
loop around vk_trace_rays' per-ray streams does differ with media (otherwise this would show nothing), and without media the two loops
agree bounce by bounce.  The compaction's numpy restatement is property-tested against itself and against a plain loop.
tests/test_gpu_paths.py runs the same scenes and rays on the device."""
import numpy as np
import pytest

import paths_ref as P
import shade_ref as S
from vecchio_amd import ffi
from vecchio_amd.scene import make_path_states


@pytest.fixture(scope="session")
def emu_paths(built):
    import emu_paths_ffi
    emu_paths_ffi.load()
    return emu_paths_ffi


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


# ---------------------------------------------------------------- the compaction's reference
@pytest.mark.parametrize("n", P.SIZES)
def test_compaction_reference_properties(n):
    for name, status in P.patterns(n).items():
        items, ids, n_ids = P.items_for(status)
        rays, states, ids_out, rstate, rstatus, counts = P.compact(items, ids, n_ids)
        go = status == ffi.VK_SHADE_SCATTERED
        m = int(go.sum())
        what = f"n {n}, {name}"
        assert int(counts.sum()) == n and int(counts[1]) == m, what
        assert [int(c) for c in counts] == [int((status == s).sum()) for s in range(5)], what
        # the survivors in order, nothing beyond them
        assert (np.diff(ids_out[:m].astype(np.int64)) > 0).all() and set(ids_out[:m].tolist()) == set(ids[go].tolist()), what
        for a in (rays, states, ids_out):
            assert (a[m:].view(np.uint8) == P.CANARY).all(), what
        # a result slot is written exactly for a retired id
        written = ~(rstate.view(np.uint8).reshape(n_ids, 48) == P.CANARY).all(1)
        assert set(np.flatnonzero(written).tolist()) == set(ids[~go].tolist()), what
        assert (rstatus[ids[~go]] == status[~go]).all(), what
        # idempotent on its own survivors: compacting them again (all scattered) moves nothing
        again = np.zeros(m, items.dtype)
        again["next"], again["state"], again["status"] = rays[:m], states[:m], ffi.VK_SHADE_SCATTERED
        r2, s2, i2, _, _, c2 = P.compact(again, ids_out[:m], n_ids)
        assert r2.tobytes() == rays[:m].tobytes() and s2.tobytes() == states[:m].tobytes() and i2.tobytes() == ids_out[:m].tobytes(), what
        assert int(c2[1]) == m


@pytest.mark.parametrize("n", [1, 65, 257])
def test_compaction_reference_against_a_plain_loop(n):
    for name, status in P.patterns(n).items():
        items, ids, n_ids = P.items_for(status, seed=3)
        got = P.compact(items, ids, n_ids)
        rays, states, ids_out, rstate, rstatus = [np.zeros(len(a), a.dtype) for a in got[:5]]
        for a in (rays, states, ids_out, rstate, rstatus):
            a.view(np.uint8)[:] = P.CANARY
        m = 0
        for i in range(n):
            if status[i] == ffi.VK_SHADE_SCATTERED:
                rays[m], states[m], ids_out[m] = items["next"][i], items["state"][i], ids[i]
                m += 1
            else:
                rstate[ids[i]], rstatus[ids[i]] = items["state"][i], status[i]
        P.assert_same(got[:5], (rays, states, ids_out, rstate, rstatus), f"n {n}, {name}")


# ---------------------------------------------------------------- THE CONTRACT, media included
@pytest.mark.parametrize("kind,name", S.ALL_SCENES, ids=[f"{k}-{n}" for k, n in S.ALL_SCENES])
def test_loop_on_scene(kind, name, emu_paths, emu_queries, host_scenes):
    """max_depth 8 with 1 sample, max_depth 50 with samples 0..2: the batch stepped to its end is the radiance query's sample"""
    desc, cam, p = S.scene(kind, name, host_scenes)
    rays = S.rays_of(cam)
    integrators = S.integrators(desc)
    assert integrators
    for integrator in integrators:
        for depth, spp in ((8, 1), (50, 3)):
            what = f"{kind} {name}, integrator {integrator}, max_depth {depth}"
            want, _ = emu_queries.radiance_samples(desc, rays, **S.radiance_kwargs(p, integrator, depth, samples_per_ray=spp))
            for s in range(spp):
                got, bounces = emu_paths.run(desc, rays, S.SEED, S.FIRST, s, **S.shade_kwargs(p, integrator, depth))
                assert 1 <= len(bounces) <= depth, what
                for ids, _, _ in bounces:
                    assert (np.diff(ids.astype(np.int64)) > 0).all(), what
                S.assert_samples_equal(got, want[:, s], f"{what}, sample {s}")
            assert want[..., 3].view(np.uint32).max() > 0, what


def test_the_per_ray_stream_loop_does_differ_with_media(emu_paths, emu_shade, emu_queries, host_scenes):
    """the loop around vk_trace_rays — a medium's distance from the ray's own stream — is NOT the radiance query's sample in a scene with
    a ConstantMedium, where the path batch's is: what test_loop_on_scene shows there is the path stream"""
    plain, media = S.split_by_media(host_scenes)
    assert len(media) >= 2
    differs = []
    for kind, name in media:
        desc, cam, p = S.scene(kind, name, host_scenes)
        rays = S.rays_of(cam)
        integrator = S.integrators(desc)[0]
        want, _ = emu_queries.radiance_samples(desc, rays, **S.radiance_kwargs(p, integrator, 8))
        old, _ = emu_shade.wavefront(desc, rays, S.SEED, S.FIRST, 0, **S.shade_kwargs(p, integrator, 8))
        new, _ = emu_paths.run(desc, rays, S.SEED, S.FIRST, 0, **S.shade_kwargs(p, integrator, 8))
        S.assert_samples_equal(new, want[:, 0], f"{kind} {name}")
        if not np.array_equal(old.view(np.uint32), want[:, 0].view(np.uint32)):
            differs.append((kind, name))
    assert differs, "no media scene tells the two loops apart"


def test_without_media_the_two_loops_agree_bounce_by_bounce(emu_paths, emu_shade, host_scenes):
    """the second contract on the emulators: after every bounce the live ids, rays and states are the survivors of wavefront_loop"""
    plain, _ = S.split_by_media(host_scenes)
    for kind, name in plain[:4] + [("shade", "everything_lit")]:
        desc, cam, p = S.scene(kind, name, host_scenes)
        rays = S.rays_of(cam)
        kw = S.shade_kwargs(p, S.integrators(desc)[0], 8)
        _, want = emu_shade.wavefront(desc, rays, S.SEED, S.FIRST, 0, **kw)
        _, got = emu_paths.run(desc, rays, S.SEED, S.FIRST, 0, **kw)
        assert len(got) == len(want), (kind, name)
        for k, ((ids, r, s), b) in enumerate(zip(got, want)):
            go = b["out"]["status"] == ffi.VK_SHADE_SCATTERED
            assert np.array_equal(ids, b["index"][go]), (kind, name, k)
            assert r.tobytes() == np.ascontiguousarray(b["out"]["next"][go]).tobytes(), (kind, name, k)
            assert s.tobytes() == np.ascontiguousarray(b["out"]["state"][go]).tobytes(), (kind, name, k)


def test_cull_and_results_on_the_emulator(emu_paths, host_scenes):
    """the emulator batch's cull and mid-loop results mean what the header says (tests/test_gpu_paths.py compares the device with it)"""
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    rays = S.rays_of(cam)
    b = emu_paths.Batch(desc, **S.shade_kwargs(p, p.integrator, 8))
    b.begin(rays, make_path_states(len(rays), S.SEED, S.FIRST, 0))
    b.step(); b.step()
    ids, _, states = b.read()
    assert len(ids) > 8
    keep = (np.arange(len(ids)) % 2 == 0).astype(np.uint8)
    scale = np.linspace(0.5, 2.0, len(ids)).astype(np.float32)
    b.cull(keep, scale)
    ids2, _, states2 = b.read()
    assert np.array_equal(ids2, ids[keep != 0])
    assert np.array_equal(states2["thr"], (states["thr"][keep != 0] * scale[keep != 0, None]).astype(np.float32))
    rs, rst = b.results()
    assert (rst[ids[keep == 0]] == ffi.VK_PATHS_CULLED).all() and rs[ids[keep == 0]].tobytes() == states[keep == 0].tobytes()
    assert (rst[ids2] == ffi.VK_PATHS_LIVE).all() and rs[ids2].tobytes() == states2.tobytes()
    assert int(b.retired[ffi.VK_PATHS_CULLED]) == int((keep == 0).sum())
