"""Films on the CPU: vk_film_emit's camera paths (vk_trace.h start_sample_core through tests/emu/emu_film.cpp) run through the emulator
loop of a path batch, per sample against the render emulator — radiance and stream counter bit for bit — and against the oracle (equal
draw counts, equal finite masks, radiance within the emulator-against-oracle tolerance of tests/test_emu_parity.py), on every scene of the
shade tests' set and each integrator vk_render allows there, at the scene's own small frame and 3 samples per pixel; the deposit in C++
and in numpy against tests/exact_sums.py's image of the dump; a lens with an aperture and a shutter over moving spheres; windows.
tests/test_gpu_film.py runs the same scenes on the device."""
import numpy as np
import pytest

import exact_sums as E
import film_ref as F
import shade_ref as S
from descs import camera
from vecchio_amd import ffi

SPP = 3


@pytest.fixture(scope="session")
def emu_film(built):
    import emu_film_ffi
    emu_film_ffi.load()
    return emu_film_ffi


def frame_params(p, integrator, spp=SPP, max_depth=None):
    q = ffi.RenderParams.from_buffer_copy(p)
    q.samples_per_pixel, q.integrator = spp, integrator
    if max_depth is not None:
        q.max_depth = max_depth
    return q


def as_samples(states):
    res = np.zeros((len(states), 4), np.float32)
    res[:, :3] = states["acc"]
    res[:, 3] = np.ascontiguousarray(states["counter"]).view(np.float32)
    return res


def compare_with_oracle(ps_o, ps_e):
    """tests/test_emu_parity.py compare(), per sample"""
    d_o, d_e = ps_o[:, 3].view(np.uint32), ps_e[:, 3].view(np.uint32)
    assert np.array_equal(d_o, d_e), f"{int((d_o != d_e).sum())} samples took a different path (draw counts differ)"
    fo, fe = np.isfinite(ps_o[:, :3]).all(1), np.isfinite(ps_e[:, :3]).all(1)
    assert np.array_equal(fo, fe), "finite filter (main.rs:192-194) would drop different samples"
    a, b = ps_o[fo, :3], ps_e[fo, :3]
    rel = np.abs(a - b) / (np.abs(a) + 1e-3)
    assert rel.size == 0 or rel.max() < 2e-5, f"per-sample radiance differs by {rel.max()}"


@pytest.mark.parametrize("kind,name", S.ALL_SCENES, ids=[f"{k}-{n}" for k, n in S.ALL_SCENES])
def test_frame_on_scene(kind, name, emu, oracle, emu_film, host_scenes):
    desc, cam, p = S.scene(kind, name, host_scenes)
    integrators = S.integrators(desc)
    assert integrators
    for integrator in integrators:
        q = frame_params(p, integrator)
        what = f"{kind} {name}, integrator {integrator}"
        _, dump, _, _ = emu.render_samples(desc, cam, q)
        states, status = emu_film.run(desc, cam, q, integrator, q.max_depth)
        assert np.isin(status, (ffi.VK_SHADE_MISS, ffi.VK_SHADE_ENDED)).all(), what
        where = F.dump_index(q.width, SPP, 0, 0, q.width, q.height, 0, SPP)
        assert np.array_equal(where, np.arange(q.width * q.height * SPP))          # the whole frame in one window: the dump's own order
        got = as_samples(states)
        S.assert_samples_equal(got, dump[where], what)
        _, dump_o = oracle.render_samples(desc, cam, q)
        compare_with_oracle(dump_o[where], got)
        # the deposit, in C++ and in numpy, resolved: the image the dump must give
        want_img, want_clamped = E.exact_image(dump, q.width, q.height, SPP)
        for dep in (emu_film.deposit, F.deposit):
            sums, c = dep(states, status, q.width, q.height, SPP)
            assert np.array_equal(sums, E.frame_sums(dump, q.width, q.height, SPP)[0]), what
            assert np.array_equal(E.resolve(sums, SPP).view(np.uint32), want_img.view(np.uint32)), what
            finite = np.isfinite(dump[:, :3]).all(1)
            assert c == dict(deposited=int(finite.sum()), dropped=int((~finite).sum()), clamped=want_clamped, skipped=0), what


def test_a_lens_and_a_shutter_over_moving_spheres(emu, emu_film, host_scenes):
    """aperture > 0: the lens disk's rejection loop runs, so the emitted counters are not all equal; time0 < time1 over moving spheres"""
    hs, _ = host_scenes("final_scene")
    assert hs.desc.contents.n_moving_spheres > 0
    cam = camera((478, 278, -600), (278, 278, 0), vfov=40.0, aspect=24 / 16, aperture=8.0, focus=600.0, t0=0.25, t1=1.0)
    assert cam.lens_radius > 0 and cam.time0 < cam.time1
    p = hs.params(24, SPP, 12, seed=11, height=16)
    rays, states = emu_film.emit(cam, p, 0, 0, 24, 16, 0, SPP)
    assert len(set(states["counter"].tolist())) > 1 and states["counter"].min() >= 5       # u, v, two or more for the disk, the time
    assert (rays["time"] >= 0.25).all() and (rays["time"] < 1.0).all() and len(set(rays["time"].tolist())) > 100
    assert len({tuple(o) for o in rays["origin"].tolist()}) > 100                             # the origin moves over the lens
    assert np.isinf(rays["tmax"]).all() and (states["depth"] == 1).all() and (states["thr"] == 1).all() and not states["acc"].any()
    pixel, sample = F.ids_of(24, 0, 0, 24, 16, 0, SPP)
    assert np.array_equal(states["pixel"], pixel) and np.array_equal(states["sample"], sample) and (states["seed"] == 11).all()
    _, dump, _, _ = emu.render_samples(hs.desc, cam, p)
    got, status = emu_film.run(hs.desc, cam, p, p.integrator, p.max_depth)
    S.assert_samples_equal(as_samples(got), dump, "final_scene through a lens")
    assert dump[:, 3].view(np.uint32).min() >= 5


def test_windows_cover_the_frame_in_any_order(emu, emu_film, host_scenes):
    """windows of a frame, sample ranges split, deposited in a shuffled order: the sums of the one-window frame"""
    desc, cam, p = S.scene("builder", "cornell_box", host_scenes)
    q = frame_params(p, p.integrator, max_depth=8)
    _, dump, _, _ = emu.render_samples(desc, cam, q)
    W, H = q.width, q.height
    wins = [(0, 0, 7, H, 0, 1), (7, 0, W - 7, 5, 0, 1), (7, 5, W - 7, H - 5, 0, 1), (0, 0, W, 3, 1, 2), (0, 3, 11, H - 3, 1, 2),
            (11, 3, W - 11, H - 3, 1, 1), (11, 3, W - 11, H - 3, 2, 1)]
    rng = np.random.default_rng(3)
    sums, total = None, dict(deposited=0, dropped=0, clamped=0, skipped=0)
    seen = np.zeros(W * H * SPP, int)
    for k in rng.permutation(len(wins)):
        states, status = emu_film.run(desc, cam, q, q.integrator, q.max_depth, window=wins[k])
        where = F.dump_index(W, SPP, *wins[k])
        seen[where] += 1
        S.assert_samples_equal(as_samples(states), dump[where], f"window {wins[k]}")
        sums, c = emu_film.deposit(states, status, W, H, SPP, sums)
        total = {key: total[key] + c[key] for key in total}
    assert (seen == 1).all()
    want, clamped = E.frame_sums(dump, W, H, SPP)
    assert np.array_equal(sums, want) and total["clamped"] == clamped and total["deposited"] + total["dropped"] == W * H * SPP


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_the_two_deposits_agree_on_the_special_cases(n, emu_film):
    """C++ against numpy on the patterns tests/test_gpu_film.py gives the device: every special radiance, pixels outside the frame, every
    status"""
    W, H = 9, 5
    for spp in (1, 3, 40):                                   # 40: the clamp is 1.3e11 / 40, below 1e10
        for name, pixel in F.pixel_patterns(n, W * H).items():
            states = F.states_for(pixel, F.radiances(n, spp, seed=len(name)))
            status = np.resize(np.array([0, 2, 4, 2, 0, 3, 2, 1, 4, 2, 7], np.uint32), n)
            a, ca = emu_film.deposit(states, status, W, H, spp)
            b, cb = F.deposit(states, status, W, H, spp)
            assert np.array_equal(a, b) and ca == cb, (n, spp, name, ca, cb)
            assert sum(ca[k] for k in ("deposited", "dropped", "skipped")) == n
    acc = F.radiances(257, 3)
    assert np.isnan(acc).any() and np.isinf(acc).any() and (np.abs(acc[np.isfinite(acc)]) > 1e10).any() and (acc == np.float32(31.999)).any()
