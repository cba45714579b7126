"""Reconstruction filters of the DEVICE against tests/splat_laws_ref.py — the operation in f64 as a gather, written from its meaning —
through the public calls DeviceScene.splat / deposit(positions) / resolve and the debug_sums hook, in both kernel forms: a. random
positions, c. the reproduction laws on a symmetric lattice, e. a sparse frame under negative lobes, and d. the state's own position
against where the emitted camera ray went (film.emit + pb.read() + step on a scene whose rays all reach the sky).  Every bound is the one
tests/splat_laws_ref.py derives; nothing is compared with tests/splat_ref.py here (bit equality with it is tests/test_gpu_splat.py's).
Run with -s for the device's own ratios.

Sizes: random and sparse inputs of 1386 samples on 21x13, 1x1, 3x2 and 64x5, cut into batches of 1, 63, 65, 257 and 1000; one sample per
pixel of a 300x7 frame in row order (a TILED workgroup of 256 lanes spans a row end there, its 260x5 tile cut by the frame on three
sides); lattices of 64 samples per pixel on frames of at most 21x13."""
import numpy as np
import pytest

import splat_laws_ref as L
import test_splat_laws as T
from descs import params
from test_gpu_splat import FORMS, dead_rays
from vecchio_amd import DeviceScene, ffi

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
LENGTHS = (1, 63, 65, 257, 1000)
WIDE = (300, 7)
KW = dict(max_depth=8, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SOLID, background_color=(0.0, 0.0, 0.0))
WORST = {}


def note(sp, ratio):
    k = T.KIND_NAMES[sp[0]]
    WORST[k] = max(WORST.get(k, 0.0), ratio)


@pytest.fixture(scope="module")
def scene(device):
    d, desc = T.far_scene()
    ds = DeviceScene(desc)
    yield ds
    ds.close()


def cuts_of(n):
    """n samples cut into batches of LENGTHS, the rest in one batch more"""
    out, at = [], 0
    for length in LENGTHS:
        if at < n:
            out.append((at, min(n, at + length)))
            at = out[-1][1]
    return out + ([(at, n)] if at < n else [])


def deposit_all(acc, pb, form, acc_rgb, W, H, pos):
    """the samples staged batch by batch the way tests/test_gpu_splat.py stages them and deposited at `pos`: (sums, contributions, image)"""
    states, _ = T.finished(acc_rgb, W, H)
    acc.reset()
    acc.debug_form(form)
    for lo, hi in cuts_of(len(states)):
        pb.begin(dead_rays(hi - lo), states[lo:hi], **KW)
        pb.cull(np.zeros(hi - lo, np.uint8))
        acc.deposit(pb, pos[lo:hi])
    inf = acc.info()
    assert inf.deposited == len(states) and inf.skipped == 0 and inf.dropped == 0
    return acc.debug_sums(), int(inf.contributions), acc.resolve()


def splat_of(ds, W, H, spp, sp):
    return ds.splat(W, H, spp, filter=sp[0], radius=sp[1], b=sp[2], c=sp[3])


# ================================================================ a. random positions
def random_inputs(W, H):
    if (W, H) == WIDE:                                     # one sample per pixel, in row order
        n = W * H
        rng = np.random.default_rng(W + H)
        pos = np.stack([np.arange(n) % W + rng.random(n), np.arange(n) // W + rng.random(n)], axis=1).astype(f32)
        pos = np.minimum(pos, np.array([T.below(W), T.below(H)], f32))
    else:
        n = sum(LENGTHS)
        pos = T.random_positions(W, H, n, seed=W * 100 + H)
    return pos, T.radiances(n, seed=W + H)


@pytest.mark.parametrize("sp", T.SETTINGS, ids=T.SETTING_IDS)
def test_random_positions(sp, scene):
    worst = share = 0.0
    with scene.paths(1000) as pb:
        for W, H in L.FRAMES + [WIDE]:
            pos, rgb = random_inputs(W, H)
            cf = L.gather(sp, pos, rgb, W, H)
            assert cf.st.marginal_share() <= L.MAX_MARGINAL
            share = max(share, cf.st.marginal_share())
            with splat_of(scene, W, H, T.SPP, sp) as acc:
                for form in FORMS:
                    sums, contributions, image = deposit_all(acc, pb, form, rgb, W, H, pos)
                    what = f"device form {form} {sp} {W}x{H}"
                    worst = max(worst, L.assert_sums(cf, sums, contributions, what), L.assert_image(cf, image, what)[0])
    note(sp, worst)
    print(f"\n   device, random positions {sp}: worst deviation / bound {worst:.3g}, marginal triples {share:.2e}")


# ================================================================ c. reproduction laws
LATTICE_FRAMES = [(21, 13), (1, 1), (3, 2)]
LATTICE_SETTINGS = [(s, i) for s, i in zip(T.SETTINGS, T.SETTING_IDS) if s[1] in L.RADII]


@pytest.mark.parametrize("sp", [s for s, _ in LATTICE_SETTINGS], ids=[i for _, i in LATTICE_SETTINGS])
def test_reproduction_laws(sp, scene):
    worst = 0.0
    with scene.paths(64 * 21 * 13) as pb:                  # cuts_of() leaves the rest of a lattice in one batch
        for W, H in LATTICE_FRAMES:
            pos = T.lattice(W, H)
            with splat_of(scene, W, H, 64, sp) as acc:
                for name, rgb in T.lattice_radiances(pos, W).items():
                    cf = L.gather(sp, pos, rgb, W, H)
                    assert cf.st.marginal_triples == 0 and cf.judged.all()
                    for form in FORMS:
                        sums, contributions, image = deposit_all(acc, pb, form, rgb, W, H, pos)
                        what = f"device form {form} {sp} {W}x{H} {name}"
                        worst = max(worst, L.assert_sums(cf, sums, contributions, what),
                                    T.check_lattice(sp, W, H, name, rgb, cf, image, what))
    note(sp, worst)
    print(f"\n   device, reproduction laws {sp}: worst deviation / bound {worst:.3g}, nothing marginal, nothing unjudged")


# ================================================================ d. the state's own position
@pytest.mark.parametrize("sp", T.RAY_SETTINGS, ids=["box0.5", "tent1.5", "mitchell", "catmull"])
def test_the_states_own_position_is_where_its_ray_went(sp, scene):
    W, H, spp = T.RAY_W, T.RAY_H, T.RAY_SPP
    n = W * H * spp
    p = params(W, H, spp, seed=T.RAY_SEED, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SKY)
    worst = 0.0
    with scene.film(T.rolled_camera(), p) as film, scene.paths(n) as pb, splat_of(scene, W, H, spp, sp) as acc:
        for form in FORMS:
            got = []
            for given in (False, True):
                film.emit(pb, 0, 0, W, H, 0, spp)
                ids, rays, _ = pb.read()
                assert sorted(ids.tolist()) == list(range(n))
                rays = rays[np.argsort(ids)]
                pos, slack = T.positions_of_rays(rays["origin"], rays["direction"], W, H)
                assert pb.step(100000).live == 0
                states, status = pb.results()
                assert (status == ffi.VK_SHADE_MISS).all() and (states["acc"] > 0).all()
                acc.reset()
                acc.debug_form(form)
                acc.deposit(pb, pos if given else None)
                inf = acc.info()
                assert inf.deposited == n
                got.append((acc.debug_sums(), int(inf.contributions)))
            w, share = T.check_ray_positions(sp, W, H, states["acc"], pos, slack, got[0], got[1], f"device form {form} {sp}")
            worst = max(worst, w)
    note(sp, worst)
    print(f"\n   device, own positions {sp}: worst deviation / bound {worst:.3g}; positions known to {slack[0]:.2e}, {slack[1]:.2e} px, "
          f"marginal triples under that slack {share:.2e}")


# ================================================================ e. sparse, negative lobes
@pytest.mark.parametrize("frame", L.FRAMES, ids=[f"{w}x{h}" for w, h in L.FRAMES])
def test_sparse_negative_lobes(frame, scene):
    W, H = frame
    pos, rgb, cf = T.sparse_case(W, H)
    unjudged = float((~cf.judged & ~cf.black).mean())
    assert unjudged <= L.MAX_UNJUDGED
    worst = 0.0
    with scene.paths(1000) as pb, splat_of(scene, W, H, 1, T.CATMULL) as acc:
        for form in FORMS:
            sums, contributions, image = deposit_all(acc, pb, form, rgb, W, H, pos)
            what = f"device form {form} {W}x{H}"
            worst = max(worst, L.assert_sums(cf, sums, contributions, what), L.assert_image(cf, image, what)[0])
    note(T.CATMULL, worst)
    print(f"\n   device, sparse Catmull-Rom {W}x{H}: worst deviation / bound {worst:.3g}, unjudged {unjudged:.3f}, "
          f"black by negative weight {int((cf.sums[..., 3] < -cf.bound[..., 3]).sum())} pixels")


def test_worst_ratios_of_this_run():
    print("\n   worst deviation / bound per kind, device: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
