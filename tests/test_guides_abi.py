"""Specular guides (vk_render_guides, additive symbols of ABI 7) on the CPU: declared, exported by both libraries, bound, declared in the
Rust shim; the defaults; every argument the header says is refused, refused without a device and with a message; the kernel's
register budget."""
import ctypes as C
import os
import re

import pytest

from descs import params
from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("vk_guide_default_params", "vk_render_guides", "vk_render_guides_device")


def test_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vecchio_amd.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 7\b", hdr)
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef struct vk_guide_params \{\s*uint32_t max_bounces;\s*float fuzz_max;\s*uint32_t flags;\s*\} vk_guide_params;", body)
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    for name in SYMS:
        assert re.search(rf"\bint {name}\s*\(", body), name
        assert hasattr(C.CDLL(ffi.device_lib_path()), name), name
        assert hasattr(C.CDLL(build.build_device_debug()), name), name
        assert name in ffi.DEVICE_SYMBOLS
        assert re.search(rf"pub fn {name}\(", rs), name
    assert "pub struct vk_guide_params" in rs
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == 7
    common = [C.c_void_p, C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.c_uint32, C.POINTER(ffi.GuideParams)]
    assert lib.vk_render_guides.argtypes == common + [C.c_void_p] * 5 + [C.POINTER(ffi.Stats)]
    assert lib.vk_render_guides_device.argtypes == common + [C.c_void_p] * 6 + [C.POINTER(ffi.Stats)]
    assert C.sizeof(ffi.GuideParams) == 12


def test_defaults(built):
    lib = ffi.load_device_lib()
    gp = ffi.GuideParams(99, -1.0, 7)
    assert lib.vk_guide_default_params(C.byref(gp)) == ffi.VK_OK
    assert (gp.max_bounces, gp.fuzz_max, gp.flags) == (4, 0.0, 0)
    assert lib.vk_guide_default_params(None) == ffi.VK_ERR_BAD_ARG
    assert b"null" in lib.vk_last_error()


BAD = [("max_bounces", 9, b"max_bounces"), ("fuzz_max", -0.25, b"fuzz_max"), ("fuzz_max", float("inf"), b"fuzz_max"),
       ("fuzz_max", float("nan"), b"fuzz_max"), ("flags", 1, b"flags")]


@pytest.mark.parametrize("field,value,word", BAD)
def test_bad_guide_params_refused_without_a_device(field, value, word, built):
    lib = ffi.load_device_lib()
    cam, p = ffi.Camera(), params(16, 16, 1)
    buf = (C.c_float * (16 * 16 * 3))()
    gp = ffi.GuideParams()
    lib.vk_guide_default_params(C.byref(gp))
    setattr(gp, field, value)
    # (a scene handle that is never read: the guide parameters are checked first)
    assert lib.vk_render_guides(None, C.byref(cam), C.byref(p), 0, C.byref(gp), buf, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
    assert word in lib.vk_last_error(), lib.vk_last_error()
    assert lib.vk_render_guides_device(None, C.byref(cam), C.byref(p), 0, C.byref(gp), buf, None, None, None, None, None,
                                       None) == ffi.VK_ERR_BAD_ARG
    assert word in lib.vk_last_error(), lib.vk_last_error()


def test_null_arguments_refused_without_a_device(built):
    lib = ffi.load_device_lib()
    cam, p = ffi.Camera(), params(16, 16, 1)
    buf = (C.c_float * (16 * 16 * 3))()
    gp = ffi.GuideParams()
    lib.vk_guide_default_params(C.byref(gp))
    # five NULL buffers
    assert lib.vk_render_guides(None, C.byref(cam), C.byref(p), 0, C.byref(gp), None, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
    assert b"all five" in lib.vk_last_error()
    assert lib.vk_render_guides_device(None, C.byref(cam), C.byref(p), 0, C.byref(gp), None, None, None, None, None, None,
                                       None) == ffi.VK_ERR_BAD_ARG
    assert b"all five" in lib.vk_last_error()
    # bounces alone is a wanted buffer: the call gets as far as the null scene
    assert lib.vk_render_guides(None, C.byref(cam), C.byref(p), 0, C.byref(gp), None, None, None, None, buf, None) == ffi.VK_ERR_BAD_ARG
    assert b"null argument" in lib.vk_last_error()
    # null guide parameters
    assert lib.vk_render_guides(None, C.byref(cam), C.byref(p), 0, None, buf, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
    assert b"null guide" in lib.vk_last_error()


def _resources(pattern):
    txt = open(build.kernel_resources_path()).read()
    out = {}
    for blk in txt.split("Name: ")[1:]:
        name = blk.split("\n")[0].strip()
        m = re.search(pattern, name)
        if not m:
            continue
        get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
        out[int(m.group(1))] = dict(vgprs=get("VGPRs"), agprs=get("AGPRs"), scratch=get("ScratchSize [bytes/lane]"),
                                    occupancy=get("Occupancy [waves/SIMD]"), dynamic_stack="Dynamic Stack: True" in blk,
                                    lds=get("LDS Size [bytes/block]"), scratch_ops=get("ScratchOps"))
    return out


def test_guides_kernel_budget(built):
    v = _resources(r"specular_guides_kernelILj(\d+)E")
    # two instances: sphere-only worlds and the everything-variant (VKF_ALL_SCENE = 0x17F)
    assert set(v) == {0, 0x17F}, sorted(v)
    for r in v.values():
        # no recursion, no LDS, no AGPRs
        assert not r["dynamic_stack"] and r["lds"] == 0 and r["agprs"] == 0, r
    # sphere-only: 69 VGPRs measured, 7 waves per SIMD — aov_kernel<0>'s occupancy.  96 B of private memory: the spilled SGPRs' lanes,
    # and the 17 dwords parked on purpose (thr, len, the delta hit's normal and b across a walk; the running sums between samples),
    # all written and read outside the traversal loop — as flat loads and stores to the private aperture, not scratch_* instructions,
    # which is why ScratchOps reads 0 and cannot watch them.  In registers they cost 83 VGPRs and 5 waves.
    assert v[0]["vgprs"] <= 72 and v[0]["occupancy"] >= 7 and v[0]["scratch"] <= 96, v[0]
    # everything-variant: 123 VGPRs, 4 waves per SIMD (147 and 3 without the parking); 176 B of private memory: the SpecDiffuse
    # stack's 112 and the parked state
    assert v[0x17F]["vgprs"] <= 128 and v[0x17F]["occupancy"] >= 4 and v[0x17F]["scratch"] <= 176, v[0x17F]
    # the first-hit kernel's instances are what they were (tests/test_aov_abi.py pins them); the name does not count as one of them
    # the compiler spills nothing of its own: the scratch_* instructions are the SpecDiffuse stack's, as in aov_kernel
    assert v[0]["scratch_ops"] == 0 and v[0x17F]["scratch_ops"] <= 2, v
    a = _resources(r"(?<![a-z_])aov_kernelILj(\d+)E")
    assert set(a) == {0, 0x17F}
    assert a[0]["vgprs"] == 69 and a[0x17F]["vgprs"] == 124, a
