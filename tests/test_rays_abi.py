"""Ray queries (vk_trace_rays, additive symbols of ABI 7) on the CPU: declared, exported by both libraries, bound, declared in the Rust
shim; the three structs' sizes and offsets as gcc lays them out against the ctypes mirror; every argument the header says is refused,
refused without a device; the kernel's register budget."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from vecchio_amd import build, ffi
from vecchio_amd.scene import HIT_DTYPE, RAY_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("vk_trace_rays", "vk_trace_rays_device")
STRUCTS = {"vk_ray": ffi.Ray, "vk_hit": ffi.Hit, "vk_trace_params": ffi.TraceParams}


def test_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vecchio_amd.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 7\b", hdr)
    assert re.search(r"#define VK_RAY_TMIN 0\.001f", hdr) and ffi.VK_RAY_TMIN == 0.001
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    for name in SYMS:
        assert re.search(rf"\bint {name}\s*\(", body), name
        assert hasattr(C.CDLL(ffi.device_lib_path()), name), name
        assert hasattr(C.CDLL(build.build_device_debug()), name), name
        assert name in ffi.DEVICE_SYMBOLS
        assert re.search(rf"pub fn {name}\(", rs), name
    for name in STRUCTS:
        assert f"pub struct {name}" in rs
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == 7
    assert lib.vk_trace_rays.argtypes == [C.c_void_p, C.POINTER(ffi.TraceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(ffi.Stats)]
    assert lib.vk_trace_rays_device.argtypes == [C.c_void_p, C.POINTER(ffi.TraceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                 C.POINTER(ffi.Stats)]
    assert lib.vk_trace_rays.restype is C.c_int and lib.vk_trace_rays_device.restype is C.c_int


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """sizes 32 / 64 / 24 and every field's offset and size: the header through gcc against the ctypes mirror and the numpy dtypes"""
    lines = []
    for cname, T in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in T._fields_:
            lines.append(f'printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname} *)0)->{f}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vecchio_amd.h"\nint main(void) {\n' + "\n".join(lines) +
                   "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    seen = {}
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if ln:
            k, *v = ln.split()
            seen[k] = tuple(int(x) for x in v)
    assert seen["vk_ray"] == (32,) and seen["vk_hit"] == (64,) and seen["vk_trace_params"] == (24,)
    for cname, T in STRUCTS.items():
        assert C.sizeof(T) == seen[cname][0]
        for f, _ in T._fields_:
            assert seen[f"{cname}.{f}"] == (getattr(T, f).offset, getattr(T, f).size), (cname, f)
    for dt, cname in ((RAY_DTYPE, "vk_ray"), (HIT_DTYPE, "vk_hit")):
        assert dt.itemsize == seen[cname][0]
        for f in dt.names:
            assert dt.fields[f][1] == seen[f"{cname}.{f}"][0], (cname, f)


def test_bad_arguments_refused_without_a_device(built):
    lib = ffi.load_device_lib()
    tp = ffi.TraceParams(1, 0, 0, 0)
    rays = np.zeros(4, RAY_DTYPE)
    hits = np.full(4, 7, np.uint8).repeat(64).view(HIT_DTYPE)
    before = hits.copy()
    st = ffi.Stats()
    st.samples = 99
    scene = C.c_void_p(0x1000)            # never read: each of these is refused first
    cases = [
        (lib.vk_trace_rays, (None, C.byref(tp), rays.ctypes.data, 4, hits.ctypes.data), b"null argument"),
        (lib.vk_trace_rays, (scene, None, rays.ctypes.data, 4, hits.ctypes.data), b"null argument"),
        (lib.vk_trace_rays, (scene, C.byref(tp), None, 4, hits.ctypes.data), b"null rays or hits"),
        (lib.vk_trace_rays, (scene, C.byref(tp), rays.ctypes.data, 4, None), b"null rays or hits"),
        (lib.vk_trace_rays, (scene, C.byref(tp), rays.ctypes.data, 2 ** 32 + 1, hits.ctypes.data), b"2^32"),
    ]
    for fn, args, word in cases:
        assert fn(*args, C.byref(st)) == ffi.VK_ERR_BAD_ARG, word
        assert word in lib.vk_last_error(), lib.vk_last_error()
        dev = args[:4] + (args[4], None)
        assert lib.vk_trace_rays_device(*dev, C.byref(st)) == ffi.VK_ERR_BAD_ARG, word
        assert word in lib.vk_last_error(), lib.vk_last_error()
    bad = ffi.TraceParams(1, 0, 1, 0)
    assert lib.vk_trace_rays(scene, C.byref(bad), rays.ctypes.data, 4, hits.ctypes.data, C.byref(st)) == ffi.VK_ERR_BAD_ARG
    assert b"flags" in lib.vk_last_error()
    assert lib.vk_trace_rays_device(scene, C.byref(bad), rays.ctypes.data, 4, hits.ctypes.data, None, C.byref(st)) == ffi.VK_ERR_BAD_ARG
    assert b"flags" in lib.vk_last_error()
    # outputs untouched
    assert st.samples == 99 and np.array_equal(hits.view(np.uint8), before.view(np.uint8))
    # no rays: VK_OK, nothing done, also with null arrays (the scene handle is not read)
    assert lib.vk_trace_rays(scene, C.byref(tp), None, 0, None, C.byref(st)) == ffi.VK_OK and st.samples == 0
    assert lib.vk_trace_rays_device(scene, C.byref(tp), None, 0, None, None, None) == ffi.VK_OK


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


def test_trace_kernel_budget(built):
    v = _resources(r"trace_rays_kernelILj(\d+)E")
    a = _resources(r"(?<![a-z_])aov_kernelILj(\d+)E")
    # two instances, aov_kernel's: sphere-only worlds and the everything-variant (VKF_ALL_SCENE = 0x17F)
    assert set(v) == {0, 0x17F} == set(a), (sorted(v), sorted(a))
    for F, r in v.items():
        # no recursion, no LDS, no AGPRs; occupancy not below the first-hit kernel's for the same F (7 and 4 waves per SIMD)
        assert not r["dynamic_stack"] and r["lds"] == 0 and r["agprs"] == 0, r
        assert r["occupancy"] >= a[F]["occupancy"], (F, r, a[F])
    assert a[0]["occupancy"] >= 7 and a[0x17F]["occupancy"] >= 4, a
    # measured: 54 VGPRs and 8 waves, 78 and 6; no private memory at all (no SpecDiffuse stack: a ray query evaluates no material)
    assert v[0]["scratch_ops"] == 0 and v[0x17F]["scratch_ops"] == 0, v
