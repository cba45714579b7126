"""Occlusion queries (vk_trace_occluded, additive symbols of ABI 7) on the CPU: declared, exported by both libraries, bound, declared in
the Rust shim; every argument the header says is refused, refused without a device; the kernels' register budget."""
import ctypes as C
import os
import re

import numpy as np

from vecchio_amd import build, ffi
from vecchio_amd.scene import RAY_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("vk_trace_occluded", "vk_trace_occluded_device")


def test_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vecchio_amd.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 7\b", hdr)
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    for name in SYMS:
        assert re.search(rf"\bint {name}\s*\(", body), name
        assert hasattr(C.CDLL(ffi.device_lib_path()), name), name
        assert hasattr(C.CDLL(build.build_device_debug()), name), name
        assert name in ffi.DEVICE_SYMBOLS
        assert re.search(rf"pub fn {name}\(", rs), name
    # the one-sentence contract and the segment rule are in the header
    flat = " ".join(hdr.split()).replace(" * ", " ")
    assert "occluded[i] equals hits[i].hit of vk_trace_rays called with the same scene, params and rays, bit for bit" in flat
    assert "origin = a, direction = b - a, tmax = 1" in flat
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == 7 == ffi.VK_ABI_VERSION
    assert lib.vk_trace_occluded.argtypes == [C.c_void_p, C.POINTER(ffi.TraceParams), C.c_void_p, C.c_uint64, C.c_void_p,
                                              C.POINTER(ffi.Stats)]
    assert lib.vk_trace_occluded_device.argtypes == [C.c_void_p, C.POINTER(ffi.TraceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                     C.POINTER(ffi.Stats)]
    assert lib.vk_trace_occluded.restype is C.c_int and lib.vk_trace_occluded_device.restype is C.c_int
    # the A/B hook: exported by both (the product library serves the production form only)
    assert hasattr(C.CDLL(build.build_device_debug()), "vk_debug_trace_occluded_device")
    assert hasattr(C.CDLL(ffi.device_lib_path()), "vk_debug_trace_occluded_device")
    dbg = open(os.path.join(ROOT, "include", "vecchio_amd_debug.h")).read()
    assert re.search(r"\bint vk_debug_trace_occluded_device\s*\(", re.sub(r"/\*.*?\*/", "", dbg, flags=re.S))


def test_bad_arguments_refused_without_a_device(built):
    lib = ffi.load_device_lib()
    tp = ffi.TraceParams(1, 0, 0, 0)
    rays = np.zeros(4, RAY_DTYPE)
    occ = np.full(4, 7, np.uint8)
    st = ffi.Stats()
    st.samples = 99
    scene = C.c_void_p(0x1000)            # never read: each of these is refused first
    cases = [
        ((None, C.byref(tp), rays.ctypes.data, 4, occ.ctypes.data), b"null argument"),
        ((scene, None, rays.ctypes.data, 4, occ.ctypes.data), b"null argument"),
        ((scene, C.byref(tp), None, 4, occ.ctypes.data), b"null rays or occluded"),
        ((scene, C.byref(tp), rays.ctypes.data, 4, None), b"null rays or occluded"),
        ((scene, C.byref(tp), rays.ctypes.data, 2 ** 32 + 1, occ.ctypes.data), b"2^32"),
        ((scene, C.byref(ffi.TraceParams(1, 0, 1, 0)), rays.ctypes.data, 4, occ.ctypes.data), b"flags"),
    ]
    for args, word in cases:
        assert lib.vk_trace_occluded(*args, C.byref(st)) == ffi.VK_ERR_BAD_ARG, word
        assert word in lib.vk_last_error(), lib.vk_last_error()
        assert lib.vk_trace_occluded_device(*args, None, C.byref(st)) == ffi.VK_ERR_BAD_ARG, word
        assert word in lib.vk_last_error(), lib.vk_last_error()
    # outputs untouched
    assert st.samples == 99 and (occ == 7).all()
    # no rays: VK_OK, nothing done, also with null arrays (the scene handle is not read)
    assert lib.vk_trace_occluded(scene, C.byref(tp), None, 0, None, C.byref(st)) == ffi.VK_OK and st.samples == 0
    assert lib.vk_trace_occluded_device(scene, C.byref(tp), None, 0, None, None, None) == ffi.VK_OK
    assert (occ == 7).all()


def _resources(pattern):
    txt = open(build.kernel_resources_path()).read()
    out = {}
    for blk in txt.split("Name: ")[1:]:
        name = blk.split("\n")[0].strip()
        m = re.search(pattern, name)
        if not m:
            continue
        get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
        out[tuple(int(g) for g in m.groups())] = dict(
            vgprs=get("VGPRs"), agprs=get("AGPRs"), scratch=get("ScratchSize [bytes/lane]"), occupancy=get("Occupancy [waves/SIMD]"),
            dynamic_stack="Dynamic Stack: True" in blk, lds=get("LDS Size [bytes/block]"), scratch_ops=get("ScratchOps"))
    return out


def test_occlusion_kernel_budget(built):
    """the product library holds one form of the kernel in two instances (sphere-only worlds, the everything-variant VKF_ALL_SCENE =
    0x17F): no private memory, no LDS, and no more VGPRs than the closest-hit kernel of the same F — nothing of the record is live"""
    occ = _resources(r"occlusion_kernelILj(\d+)ELb([01])E")
    tr = _resources(r"trace_rays_kernelILj(\d+)E")
    assert {k[0] for k in occ} == {0, 0x17F} and len(occ) == 2, sorted(occ)
    assert len({k[1] for k in occ}) == 1, sorted(occ)          # the other form is in the debug library only
    print("\n   occlusion_kernel:", occ, "\n   trace_rays_kernel:", tr)
    for (F, refill), r in occ.items():
        assert r["scratch"] == 0 and r["scratch_ops"] == 0 and not r["dynamic_stack"] and r["lds"] == 0 and r["agprs"] == 0, (F, refill, r)
        assert r["vgprs"] <= tr[(F,)]["vgprs"], (F, refill, r, tr[(F,)])


def test_the_kernel_source_has_no_lds_atomics_or_assembly():
    src = open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_kernels.h")).read()
    a = src.index("void occlusion_kernel(")
    body = src[a:src.index("// ---- tile slabs", a)]
    for word in ("__shared__", "atomic", "asm"):
        assert word not in body, word
    assert re.search(r"constexpr uint32_t OCC_K = (\d+)u, OCC_T = (\d+)u;", src)
