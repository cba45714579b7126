"""First-hit buffers (vk_render_aov, additive symbols of ABI 7) on the CPU: declared, exported by both libraries, bound, declared in the
Rust shim, refused without a device when the arguments are bad; the kernel's register budget; and self-tests of the per-sample references
(tests/aov_ref.py) on hand-built scenes with closed-form answers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aov_ref
from descs import Desc, camera, params
from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("vk_render_aov", "vk_render_aov_device")


def test_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vecchio_amd.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 7\b", hdr)
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in SYMS:
        assert re.search(rf"\bint {name}\s*\(", body), name
        assert hasattr(C.CDLL(ffi.device_lib_path()), name), name
        assert hasattr(C.CDLL(build.build_device_debug()), name), name
        assert name in ffi.DEVICE_SYMBOLS
    assert ffi.VK_ABI_VERSION == 7
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == 7
    common = [C.c_void_p, C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_uint32]
    assert lib.vk_render_aov.argtypes == common + [C.c_void_p] * 4 + [C.POINTER(ffi.Stats)]
    assert lib.vk_render_aov_device.argtypes == common + [C.c_void_p] * 5 + [C.POINTER(ffi.Stats)]
    assert lib.vk_render_aov.restype is C.c_int and lib.vk_render_aov_device.restype is C.c_int
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    for name in SYMS:
        assert re.search(rf"pub fn {name}\(", rs), name


def test_null_arguments_refused_without_a_device(built):
    lib = ffi.load_device_lib()
    cam, p = ffi.Camera(), params(16, 16, 1)
    buf = (C.c_float * (16 * 16 * 3))()
    assert lib.vk_render_aov(None, C.byref(cam), C.byref(p), 0, buf, None, None, None, None) == ffi.VK_ERR_BAD_ARG
    assert b"null" in lib.vk_last_error()
    assert lib.vk_render_aov(None, None, None, 0, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_render_aov_device(None, C.byref(cam), C.byref(p), 0, buf, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
    assert b"null" in lib.vk_last_error()


def _aov_resources():
    txt = open(build.kernel_resources_path()).read()
    out = {}
    for blk in txt.split("Name: ")[1:]:
        name = blk.split("\n")[0].strip()
        m = re.search(r"aov_kernelILj(\d+)E", name)
        if not m:
            continue
        get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
        out[int(m.group(1))] = dict(vgprs=get("VGPRs"), agprs=get("AGPRs"), scratch=get("ScratchSize [bytes/lane]"),
                                    occupancy=get("Occupancy [waves/SIMD]"), dynamic_stack="Dynamic Stack: True" in blk,
                                    lds=get("LDS Size [bytes/block]"))
    return out


def test_aov_kernel_budget(built):
    v = _aov_resources()
    # two instances only: sphere-only worlds (C2's fused sphere path) and the everything-variant (VKF_ALL_SCENE = 0x17F)
    assert set(v) == {0, 0x17F}, sorted(v)
    for r in v.values():
        # no recursion (the SpecDiffuse mix walks an explicit 8-level stack), no LDS, no AGPRs
        assert not r["dynamic_stack"] and r["lds"] == 0 and r["agprs"] == 0, r
    # sphere-only: 69 VGPRs measured, 7 waves per SIMD — the walk from global memory wants waves in flight; 52 B of scratch are the
    # spilled SGPRs' lanes and the per-launch constants, none in the traversal loop
    assert v[0]["vgprs"] <= 72 and v[0]["occupancy"] >= 7 and v[0]["scratch"] <= 64, v[0]
    # everything-variant: 124 VGPRs, 4 waves per SIMD; 112 B of scratch hold the SpecDiffuse stack (8 levels x (index + colour))
    assert v[0x17F]["vgprs"] <= 128 and v[0x17F]["occupancy"] >= 4 and v[0x17F]["scratch"] <= 128, v[0x17F]


def test_no_render_kernel_instance_added(built):
    txt = open(build.kernel_resources_path()).read()
    assert "aov_kernel" in txt
    assert not re.search(r"render_kernel[^\n]*AovArgs", txt)


# ---------------------------------------------------------------- self-tests of the references (CPU oracle)
def test_ref_solid_sphere_fills_the_view(oracle):
    d = Desc()
    red = d.lambertian(0.7, 0.2, 0.1)
    world = d.sphere((0, 0, 0), 100.0, red)
    desc = d.finish(world)
    cam = camera((0, 0, 0), (0, 0, -1), vfov=40.0)       # inside the sphere: every ray hits its far side at distance 100
    p = params(6, 6, 1, integrator=ffi.VK_INTEGRATOR_SCATTER)
    a = aov_ref.ref_a(oracle, desc, cam, p, [0, 1])
    assert (a["coverage"] == 1).all()
    np.testing.assert_allclose(a["depth"], 100.0, rtol=1e-5)
    np.testing.assert_array_equal(a["albedo"], np.broadcast_to(np.float32([0.7, 0.2, 0.1]), a["albedo"].shape))
    # inside: the face-oriented normal points back at the camera, i.e. towards the centre
    o, dd, _ = aov_ref.primary_ray(oracle, cam, p, 2, 3, 1)
    u = dd / np.linalg.norm(dd)
    np.testing.assert_allclose(a["normal"][1, 3, 2], -u, atol=1e-5)
    b = aov_ref.ref_b_albedo(oracle, desc, cam, params(6, 6, 2, integrator=ffi.VK_INTEGRATOR_SCATTER))
    np.testing.assert_allclose(b, np.broadcast_to(np.float32([0.7, 0.2, 0.1]), b.shape), atol=0)


def test_ref_checker_plane(oracle):
    d = Desc()
    chk = d.checker(d.solid(0.1, 0.2, 0.3), d.solid(0.9, 0.8, 0.7))
    m = d.mat(ffi.VK_MAT_LAMBERTIAN, chk)
    world = d.xz_rect(-50, 50, -50, 50, 0.05, m)       # sin(10 * 0.05) > 0: the sign is x's and z's
    desc = d.finish(world)
    cam = camera((0, 5, 0.01), (0, 0, 0), vfov=60.0)
    p = params(8, 8, 1, integrator=ffi.VK_INTEGRATOR_SCATTER)
    a = aov_ref.ref_a(oracle, desc, cam, p, [0])
    assert (a["coverage"] == 1).all()
    np.testing.assert_allclose(a["normal"][0], np.broadcast_to(np.float32([0, 1, 0]), (8, 8, 3)))
    # closed form: the checker's sign at the hit point, sin in f64 (away from the lines the f32 sine could round across)
    for y in range(8):
        for x in range(8):
            o, dd, _ = aov_ref.primary_ray(oracle, cam, p, x, y, 0)
            t = (0.05 - o[1]) / dd[1]
            q = o.astype(np.float64) + t * dd.astype(np.float64)
            s = np.sin(10 * q[0]) * np.sin(10 * q[1]) * np.sin(10 * q[2])
            if abs(np.sin(10 * q[0])) > 1e-3 and abs(np.sin(10 * q[2])) > 1e-3:
                want = [0.1, 0.2, 0.3] if s < 0 else [0.9, 0.8, 0.7]
                np.testing.assert_allclose(a["albedo"][0, y, x], want, rtol=1e-6)
    b = aov_ref.ref_b_albedo(oracle, desc, cam, params(8, 8, 1, integrator=ffi.VK_INTEGRATOR_SCATTER))
    np.testing.assert_allclose(b[0], a["albedo"][0], atol=1e-6)


def test_ref_sky_pixel(oracle):
    d = Desc()
    world = d.sphere((0, -1000, 0), 1.0, d.lambertian(0.5, 0.5, 0.5))     # far below the view
    desc = d.finish(world)
    cam = camera((0, 0, 0), (0, 1, -1), vfov=30.0)
    p = params(4, 4, 1, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SKY)
    a = aov_ref.ref_a(oracle, desc, cam, p, [0])
    assert (a["coverage"] == 0).all() and np.isinf(a["depth"]).all() and (a["normal"] == 0).all()
    o, dd, _ = aov_ref.primary_ray(oracle, cam, p, 1, 2, 0)
    ud = dd / np.sqrt(np.float32(dd @ dd))
    t = 0.5 * (ud[1] + 1.0)
    np.testing.assert_allclose(a["albedo"][0, 2, 1], (1 - t) * np.ones(3) + t * np.array([0.5, 0.7, 1.0]), atol=1e-6)
    b = aov_ref.ref_b_albedo(oracle, desc, cam, p)
    np.testing.assert_allclose(b[0], a["albedo"][0], atol=1e-6)


def test_ref_specdiffuse_mix(oracle):
    d = Desc()
    spec = d.mat(ffi.VK_MAT_METAL, d.solid(0.9, 0.9, 0.2), 0.0)
    diff = d.lambertian(0.1, 0.3, 0.5)
    inner = d.mat(ffi.VK_MAT_SPEC_DIFFUSE, 0, 0.25, spec, d.mat(ffi.VK_MAT_DIELECTRIC, 0, 1.5))
    mix = d.mat(ffi.VK_MAT_SPEC_DIFFUSE, 0, 0.5, inner, diff)
    world = d.sphere((0, 0, 0), 100.0, mix)
    desc = d.finish(world, [world])
    cam = camera((0, 0, 0), (0, 0, -1))
    p = params(4, 4, 1, integrator=ffi.VK_INTEGRATOR_PDF)
    f = np.float32
    inner_c = f(0.25) * f([0.9, 0.9, 0.2]) + (f(1) - f(0.25)) * f([1, 1, 1])
    want = f(0.5) * inner_c + (f(1) - f(0.5)) * f([0.1, 0.3, 0.5])
    a = aov_ref.ref_a(oracle, desc, cam, p, [0])
    np.testing.assert_array_equal(a["albedo"][0], np.broadcast_to(want, (4, 4, 3)))
    b = aov_ref.ref_b_albedo(oracle, desc, cam, p)
    np.testing.assert_array_equal(b[0], np.broadcast_to(want, (4, 4, 3)))


def test_ref_aggregation_drops_nonfinite():
    f = np.float32
    one = lambda a, n, dep, cov: dict(albedo=np.full((1, 1, 3), a, f), normal=np.full((1, 1, 3), n, f), depth=np.full((1, 1), dep, f),
                                      coverage=np.full((1, 1), cov, f))
    r = aov_ref.aggregate([one(0.5, 1.0, 2.0, 1), one(np.nan, 0.0, np.inf, 0), one(0.25, 0.0, np.inf, 0)])
    np.testing.assert_array_equal(r["albedo"], np.full((1, 1, 3), f(0.75) / f(3), f))
    np.testing.assert_array_equal(r["coverage"], np.full((1, 1), f(1) / f(3), f))
    np.testing.assert_array_equal(r["depth"], np.full((1, 1), 2.0, f))
