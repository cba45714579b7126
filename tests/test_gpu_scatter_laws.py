"""The scattering and light-sampling laws on the device: one bounce of vk_shade_hits (shade_hits_kernel) on the hand-made items of
tests/scatter_laws_ref.py, held to the f64 closed forms and the rule that tests/test_scatter_laws.py holds the emulator to — per case,
and with the items of ALL cases of a description interleaved by a fixed permutation into one batch (whose length is no multiple of 256),
so that a wave holds lanes of every material and both outcomes of every draw; the device's vk_shaded records against the emulator's byte
for byte on these inputs (non-unit normals, back faces, the lights zoo: inputs no parity test feeds it); and the traced pair through a
path batch (vk_paths_begin, vk_paths_step with max_bounces 1, vk_paths_read, vk_paths_results), which covers the batch family's shade
kernel.  Each description is built once per module; the emulator's results are computed once per case and shared."""
import numpy as np
import pytest

import scatter_laws_ref as L
from shade_ref import assert_shaded_equal
from vecchio_amd import DeviceScene, ffi
from vecchio_amd.scene import SHADED_DTYPE

pytestmark = pytest.mark.gpu
BATCHES = L.batches()


@pytest.fixture(scope="module")
def scenes(device):
    """name -> DeviceScene, one per description"""
    owners, out = [], {}
    for name, scene in L.SCENES.items():
        owner, desc = scene.desc()
        owners.append(owner)
        out[name] = DeviceScene(desc)
    yield out
    for ds in out.values():
        ds.close()


@pytest.fixture(scope="module")
def emulated(built):
    """name -> (rays, hits, states, the emulator's vk_shaded records), computed on first use and left unchanged"""
    import emu_shade_ffi
    emu_shade_ffi.load()
    cache = {}

    def get(name):
        if name not in cache:
            case = L.CASES[name]
            rays, hits, states = case.items()
            out = emu_shade_ffi.shade_hits(case.scene.desc()[1], rays, hits, states, **case.kwargs())
            for a in (rays, hits, states, out):
                a.setflags(write=False)
            cache[name] = (rays, hits, states, out)
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(L.CASES))
def test_case_on_the_device(name, scenes, emulated):
    case = L.CASES[name]
    rays, hits, states, want = emulated(name)
    out, st = scenes[case.scene.name].shade_hits(rays, hits, states, return_stats=True, **case.kwargs())
    assert st.samples == L.N and st.kernel_launches == 1
    report = case.check(out, rays, hits, states)
    print(f"\n   device {report.summary()}", end="")
    report.finish()
    assert_shaded_equal(out, want, f"{name} against the emulator")


@pytest.mark.parametrize("key", list(BATCHES), ids=[f"{s}-{L.INTEG_NAME[i]}" for s, i in BATCHES])
def test_interleaved_batch_on_the_device(key, scenes, emulated):
    names = BATCHES[key]
    parts = [emulated(name) for name in names]
    rays, hits, states, perm, slices = L.interleaved(names, parts=parts)
    assert len(rays) % 256 != 0
    back = L.unpermute(states, perm)
    for i, name in enumerate(names):               # the interleaved items ARE the cases' items
        assert back[slices[name]].tobytes() == parts[i][2].tobytes()
    out = L.unpermute(scenes[key[0]].shade_hits(rays, hits, states, **L.CASES[names[0]].kwargs()), perm)
    for i, name in enumerate(names):
        r, h, s, want = parts[i]
        mine = out[slices[name]]
        report = L.CASES[name].check(mine, r, h, s)
        print(f"\n   interleaved {report.summary()}", end="")
        report.finish()
        assert_shaded_equal(mine, want, f"{name}, interleaved, against the emulator")
    L.check_misses(out[slices[None]], back[slices[None]])


@pytest.mark.parametrize("which", list(L.TRACED))
def test_traced_pair_through_a_path_batch(which, scenes, built):
    """rays aimed at a real floor, one bounce of a path batch: the live rays and states under the same laws, the Metal case's ENDED
    count held to its share; and the bounce is vk_shade_hits' item on vk_trace_rays' hit (the emulator's, bit for bit)"""
    import emu_shade_ffi
    scene, integrator, seed, law = L.TRACED[which]
    case, ds = L.CASES[law], scenes[scene]
    rays = L.traced_rays(which)
    n = len(rays)
    states = L.make_path_states(n, seed)
    hits = ds.trace_rays(rays)
    assert (hits["hit"] == 1).all() and (hits["front"] == 1).all() and (hits["material"] == case.material).all()
    assert (hits["normal"] == np.float32([0, 1, 0])).all()
    with ds.paths(n) as pb:
        pb.begin(rays, states, **case.kwargs())
        info = pb.step(1)
        ids, live_rays, live_states = pb.read()
        final, status = pb.results()
    out = np.zeros(n, SHADED_DTYPE)
    out["state"], out["status"] = final, status
    out["next"][ids] = live_rays
    assert (status[ids] == ffi.VK_PATHS_LIVE).all() and len(ids) == (status == ffi.VK_PATHS_LIVE).sum() == n - info.ended
    assert live_states.tobytes() == final[ids].tobytes()
    report = case.check(out, rays, hits, states, has_lobe=False)
    print(f"\n   path batch {report.summary()}", end="")
    report.finish()
    want = emu_shade_ffi.shade_hits(L.SCENES[scene].desc()[1], rays, hits, states, **case.kwargs())
    out["lobe"] = want["lobe"]                     # (a path batch reports no lobe)
    assert_shaded_equal(out, want, f"{which}: a path batch's bounce against vk_shade_hits' item")
