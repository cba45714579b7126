"""Error behaviour of scene upload / render arguments.  The reference panics (unwrap, assert,
index out of bounds); across the C ABI that becomes a status code and a message.  The
lineariser is shared by the HIP library and tests/emu, so it is exercised here on the CPU."""
import ctypes as C

import numpy as np
import pytest

from descs import Desc, camera, params
from vecchio_amd import ffi


def emu_status(emu, desc, cam, p):
    lib = emu.load()
    img = np.zeros((p.height, p.width, 3), np.float32)
    return lib.emu_render(desc, C.byref(cam), C.byref(p), img.ctypes.data, None, 1, None, None), lib.emu_last_error().decode()


def test_bad_indices_rejected(emu):
    cam = camera((0, 0, -5), (0, 0, 0))
    p = params(8, 8, 1)
    d = Desc()
    d.lambertian(0.5, 0.5, 0.5)
    s = d.sphere((0, 0, 0), 1.0, 7)                       # material index out of range
    st, msg = emu_status(emu, d.finish(s, [s]), cam, p)
    assert st == ffi.VK_ERR_BAD_ARG and "material" in msg
    d = Desc()
    d.lambertian(0.5, 0.5, 0.5)
    st, msg = emu_status(emu, d.finish(ffi.make_ref(ffi.VK_KIND_SPHERE, 3)), cam, p)   # dangling reference
    assert st == ffi.VK_ERR_BAD_ARG
    d = Desc()
    s = d.sphere((0, 0, 0), 1.0, d.lambertian(0.5, 0.5, 0.5))
    desc = d.finish(s, [s])
    d.desc.abi_version = 99
    st, msg = emu_status(emu, desc, cam, p)
    assert st == ffi.VK_ERR_BAD_ARG and "abi" in msg


def test_cyclic_graph_rejected(emu):
    cam = camera((0, 0, -5), (0, 0, 0))
    p = params(8, 8, 1)
    d = Desc()
    s = d.sphere((0, 0, 0), 1.0, d.lambertian(0.5, 0.5, 0.5))
    n0 = d.big_box(s, s)
    d.bvh[0].left = n0                                   # a node that is its own child
    st, msg = emu_status(emu, d.finish(n0, [s]), cam, p)
    assert st == ffi.VK_ERR_BAD_ARG and "cyclic" in msg
    d = Desc()
    s = d.sphere((0, 0, 0), 1.0, d.lambertian(0.5, 0.5, 0.5))
    t = d.translate(s, (1, 0, 0))
    d.translates[0].child = t
    st, msg = emu_status(emu, d.finish(t, [s]), cam, p)
    assert st != ffi.VK_OK


def test_unsupported_shapes_reported(emu):
    cam = camera((0, 0, -5), (0, 0, 0))
    p = params(8, 8, 1)
    d = Desc()
    m = d.lambertian(0.5, 0.5, 0.5)
    s = d.sphere((0, 0, 0), 1.0, m)
    inner = d.big_box(s, s)
    lst = d.list_([inner])                                # a BVH inside a list: not linearisable
    st, msg = emu_status(emu, d.finish(lst, [s]), cam, p)
    assert st == ffi.VK_ERR_UNSUPPORTED and "list" in msg
    d = Desc()
    s = d.sphere((0, 0, 0), 1.0, d.lambertian(0.5, 0.5, 0.5))
    med = d.medium(d.translate(s, (1, 0, 0)), 0.5, d.mat(ffi.VK_MAT_ISOTROPIC, d.solid(1, 1, 1)))
    st, msg = emu_status(emu, d.finish(med, [s]), cam, p)
    assert st == ffi.VK_ERR_UNSUPPORTED and "boundary" in msg


def test_pdf_integrator_needs_lights(emu):
    cam = camera((0, 0, -5), (0, 0, 0))
    d = Desc()
    s = d.sphere((0, 0, 0), 1.0, d.lambertian(0.5, 0.5, 0.5))
    st, msg = emu_status(emu, d.finish(s, []), cam, params(8, 8, 1, integrator=ffi.VK_INTEGRATOR_PDF))
    assert st == ffi.VK_ERR_UNSUPPORTED and "lights" in msg   # Vec::random would unwrap None (hittable.rs:431)


def test_boxy_lists_become_compact_boxes(emu):
    """The lineariser stores an exact Boxy::new pattern as a 32-byte DBox (feature bit 0x100) and anything
    else as a generic list (0x4); both must render like the oracle (covered by the parity tests)."""
    cam = camera((5, 5, -12), (1, 1, 1))
    p = params(8, 8, 1)
    d = Desc()
    m = d.lambertian(0.5, 0.5, 0.5)
    box = d.boxy((0, 0, 0), (2, 3, 4), m)
    lm = d.light(5, 5, 5)
    ls = d.xz_rect(0, 1, 0, 1, 9, lm)
    desc = d.finish(d.big_box(box, Desc.flip(ls)), [ls])
    _, _, _, info = emu.render_samples(desc, cam, p)
    assert info[3] & 0x100 and not (info[3] & 0x4)
    d = Desc()
    m = d.lambertian(0.5, 0.5, 0.5)
    box = d.boxy((0, 0, 0), (2, 3, 4), m)
    d.rects[2].k = 2.5                                  # no longer the canonical pattern: stays a list
    lm = d.light(5, 5, 5)
    ls = d.xz_rect(0, 1, 0, 1, 9, lm)
    desc = d.finish(d.big_box(box, Desc.flip(ls)), [ls])
    _, _, _, info = emu.render_samples(desc, cam, p)
    assert info[3] & 0x4 and not (info[3] & 0x100)


# ---------------------------------------------------------------- material and texture graphs the kernel cannot resolve
# CPU only: a graph that ought to be refused is never handed to the device library, and a cyclic one never to an oracle that would
# recurse on it (the oracle's loader refuses them too: checked here through its status, which comes before any evaluation).
def _ball(d, m):
    s = d.sphere((0, 0, 0), 1.0, m)
    lm = d.light(5, 5, 5)
    ls = d.xz_rect(-1, 1, -1, 1, 3, lm)
    return d.finish(d.big_box(s, Desc.flip(ls)), [ls])


def _refused_by_both(emu, oracle, desc, status, word):
    import ctypes as C
    cam = camera((0, 0, -5), (0, 0, 0))
    p = params(8, 8, 1)
    st, msg = emu_status(emu, desc, cam, p)
    assert st == status and word in msg, (st, msg)
    lib = oracle.load()
    img = np.zeros((p.height, p.width, 3), np.float32)
    assert lib.oracle_render(desc, C.byref(cam), C.byref(p), img.ctypes.data_as(C.c_void_p), 1, None) != 0
    assert word in lib.oracle_last_error().decode()


def _checker_cycle(length, through):
    d = Desc()
    s = d.solid(0.5, 0.5, 0.5)
    ts = [d.checker(s, s) for _ in range(length)]
    for i, t in enumerate(ts):                       # t -> the next one, the last -> the first
        setattr(d.textures[t], through, ts[(i + 1) % length])
    return _ball(d, d.mat(ffi.VK_MAT_LAMBERTIAN, ts[0]))


def _spec_diffuse_cycle(length, through):
    d = Desc()
    leaf = d.lambertian(0.5, 0.5, 0.5)
    ms = [d.mat(ffi.VK_MAT_SPEC_DIFFUSE, 0, 0.5, leaf, leaf) for _ in range(length)]
    for i, m in enumerate(ms):
        field = through if through != "alternating" else "ab"[i % 2]
        setattr(d.materials[m], field, ms[(i + 1) % length])
    return _ball(d, ms[0])



@pytest.mark.parametrize("through", ["a", "b"])
@pytest.mark.parametrize("length", [1, 2])
def test_cyclic_checkers_rejected(length, through, emu, oracle):
    _refused_by_both(emu, oracle, _checker_cycle(length, through), ffi.VK_ERR_BAD_ARG, "cyclic")


@pytest.mark.parametrize("through", ["a", "b", "alternating"])
@pytest.mark.parametrize("length", [1, 2, 3])
def test_cyclic_spec_diffuse_rejected(length, through, emu, oracle):
    _refused_by_both(emu, oracle, _spec_diffuse_cycle(length, through), ffi.VK_ERR_BAD_ARG, "cyclic")


def test_a_cycle_nothing_refers_to_is_rejected_too(emu, oracle):
    d = Desc()
    t = d.checker(d.solid(1, 1, 1), d.solid(0, 0, 0))
    d.textures[t].b = t
    _refused_by_both(emu, oracle, _ball(d, d.lambertian(0.5, 0.5, 0.5)), ffi.VK_ERR_BAD_ARG, "cyclic")


def test_shared_children_are_not_a_cycle(emu):
    """a diamond: both children of a checker are the same checker, both children of a SpecDiffuse the same SpecDiffuse"""
    d = Desc()
    t = d.checker(d.solid(1, 1, 1), d.solid(0, 0, 0))
    t = d.checker(t, t)
    inner = d.mat(ffi.VK_MAT_SPEC_DIFFUSE, 0, 0.5, d.mat(ffi.VK_MAT_METAL, d.solid(0.9, 0.9, 0.9), 0.1), d.mat(ffi.VK_MAT_LAMBERTIAN, t))
    st, msg = emu_status(emu, _ball(d, d.mat(ffi.VK_MAT_SPEC_DIFFUSE, 0, 0.5, inner, inner)), camera((0, 0, -5), (0, 0, 0)), params(8, 8, 1))
    assert st == ffi.VK_OK, msg


def test_checker_chain_limit(emu, oracle):
    """the measured limit: texture_value resolves 15 checkers above a leaf and ends its loop before the leaf of 16"""
    import material_graphs as MG
    from test_emu_parity import compare
    assert MG.D_TEX == 15
    d, desc, cam, p = MG.checker_chain_scene(MG.D_TEX)
    img_o, ps_o = oracle.render_samples(desc, cam, p)
    img_e, ps_e, _, _ = emu.render_samples(desc, cam, p)
    compare(ps_o, ps_e, img_o, img_e)
    assert img_o.max() > 0
    d, desc, cam, p = MG.checker_chain_scene(MG.D_TEX + 1)
    _refused_by_both(emu, oracle, desc, ffi.VK_ERR_UNSUPPORTED, "limit")
    assert "15" in emu_status(emu, desc, cam, p)[1]


@pytest.mark.parametrize("side", ["spec", "diffuse", "mixed"])
def test_spec_diffuse_chain_limit(side, emu, oracle):
    """the measured limit: shade_core's draw loop, its scattering_pdf loop and aov_albedo's stack all resolve 8 levels"""
    import material_graphs as MG
    from test_emu_parity import compare
    assert MG.D_MAT == 8
    d, desc, cam, p = MG.spec_diffuse_chain_scene(MG.D_MAT, side)
    img_o, ps_o = oracle.render_samples(desc, cam, p)
    img_e, ps_e, _, _ = emu.render_samples(desc, cam, p)
    compare(ps_o, ps_e, img_o, img_e)
    d, desc, cam, p = MG.spec_diffuse_chain_scene(MG.D_MAT + 1, side)
    _refused_by_both(emu, oracle, desc, ffi.VK_ERR_UNSUPPORTED, "limit")
    assert "8" in emu_status(emu, desc, cam, p)[1]


def test_spec_diffuse_chain_limit_first_hit_albedo(emu, oracle):
    """aov_albedo's 8-level stack on the three limit chains, per sample against reference (a)"""
    import material_graphs as MG
    import test_aov_emu as aov_shared
    for side in ("spec", "diffuse", "mixed"):
        d, desc, cam, p = MG.spec_diffuse_chain_scene(MG.D_MAT, side)
        aov_shared.run(oracle, emu, desc, cam, p, samples=(0, 1))


NULLABLE = ("bvh", "spheres", "moving_spheres", "rects", "lists", "list_items", "media", "translates", "rotates", "materials", "textures",
            "images", "perlins", "lights")


@pytest.mark.parametrize("name", NULLABLE)
def test_null_array_with_a_count_rejected(name, emu):
    d = Desc()
    s = d.sphere((0, 0, 0), 1.0, d.lambertian(0.5, 0.5, 0.5))
    desc = _ball(d, d.lambertian(0.2, 0.2, 0.2))
    setattr(d.desc, "n_" + name, max(1, getattr(d.desc, "n_" + name)))
    setattr(d.desc, name, None)
    st, msg = emu_status(emu, desc, camera((0, 0, -5), (0, 0, 0)), params(8, 8, 1))
    assert st == ffi.VK_ERR_BAD_ARG and "null" in msg and name in msg, (st, msg)
