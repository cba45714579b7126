"""Radiance queries (vk_trace_radiance, additive symbols of ABI 7) on the CPU: declared, exported by both libraries, bound, declared in
the Rust shim; the structs' sizes and offsets as gcc lays them out against the ctypes mirror; every argument the header says is refused,
refused without a device; the new kernel's instances exist beside render_kernel's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vecchio_amd import build, ffi
from vecchio_amd.scene import KEY_DTYPE, RAY_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"vk_radiance_params": ffi.RadianceParams, "vk_debug_stream_key": ffi.DebugStreamKey}


def test_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vecchio_amd.h")).read()
    dbg = open(os.path.join(ROOT, "include", "vecchio_amd_debug.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 7\b", hdr)
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    assert re.search(r"\bint vk_trace_radiance\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert re.search(r"\bint vk_debug_trace_radiance_samples\s*\(", re.sub(r"/\*.*?\*/", "", dbg, flags=re.S))
    assert "vk_trace_radiance_device" not in hdr        # no device-pointer variant, and no stream parameter under another name
    for path in (ffi.device_lib_path(), build.build_device_debug()):
        lib = C.CDLL(path)
        assert hasattr(lib, "vk_trace_radiance") and hasattr(lib, "vk_debug_trace_radiance_samples"), path
        assert not hasattr(lib, "vk_trace_radiance_device"), path
    assert "vk_trace_radiance" in ffi.DEVICE_SYMBOLS
    assert re.search(r"pub fn vk_trace_radiance\(", rs) and "pub struct vk_radiance_params" in rs
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == 7
    assert lib.vk_trace_radiance.argtypes == [C.c_void_p, C.POINTER(ffi.RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p,
                                              C.POINTER(ffi.Stats)]
    assert lib.vk_debug_trace_radiance_samples.argtypes == [C.c_void_p, C.POINTER(ffi.RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p,
                                                            C.c_void_p, C.POINTER(ffi.Stats)]
    assert lib.vk_trace_radiance.restype is C.c_int and lib.vk_debug_trace_radiance_samples.restype is C.c_int


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """sizes 56 / 24 and every field's offset and size: the headers through gcc against the ctypes mirror and the numpy dtype"""
    lines = []
    for cname, T in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in T._fields_:
            lines.append(f'printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname} *)0)->{f}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vecchio_amd.h"\n#include "vecchio_amd_debug.h"\nint main(void) {\n' +
                   "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    seen = {}
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if ln:
            k, *v = ln.split()
            seen[k] = tuple(int(x) for x in v)
    assert seen["vk_radiance_params"] == (56,) and seen["vk_debug_stream_key"] == (24,)
    for cname, T in STRUCTS.items():
        assert C.sizeof(T) == seen[cname][0]
        for f, _ in T._fields_:
            assert seen[f"{cname}.{f}"] == (getattr(T, f).offset, getattr(T, f).size), (cname, f)
    assert KEY_DTYPE.itemsize == 24
    for f in KEY_DTYPE.names:
        assert KEY_DTYPE.fields[f][1] == seen[f"vk_debug_stream_key.{f}"][0], f


def params(**over):
    kw = dict(seed=1, first_index=0, samples_per_ray=4, first_sample=0, max_depth=5, integrator=ffi.VK_INTEGRATOR_SCATTER,
              background=ffi.VK_BACKGROUND_SKY, background_color=ffi.F3(0, 0, 0), flags=0, _pad=0)
    kw.update(over)
    return ffi.RadianceParams(**kw)


def test_bad_arguments_refused_without_a_device(built):
    lib = ffi.load_device_lib()
    rp = params()
    rays = np.zeros(4, RAY_DTYPE)
    rgb = np.full((4, 3), 7.0, np.float32)
    samples = np.full((4, 4, 4), 7.0, np.float32)
    st = ffi.Stats()
    st.samples = 99
    scene = C.c_void_p(0x1000)            # never read: each of these is refused first
    r, o, s = rays.ctypes.data, rgb.ctypes.data, samples.ctypes.data
    cases = [
        ((None, C.byref(rp), r, 4), b"null argument"),
        ((scene, None, r, 4), b"null argument"),
        ((scene, C.byref(rp), None, 4), b"null rays or output"),
        ((scene, C.byref(rp), r, 2 ** 32 + 1), b"2^32"),
        ((scene, C.byref(params(flags=1)), r, 4), b"flags"),
        ((scene, C.byref(params(samples_per_ray=0)), r, 4), b"samples_per_ray"),
        ((scene, C.byref(params(samples_per_ray=2 ** 26 + 1)), r, 4), b"samples_per_ray"),
        ((scene, C.byref(params(samples_per_ray=4, first_sample=2 ** 32 - 4)), r, 4), b"first_sample"),
        ((scene, C.byref(params(integrator=2)), r, 4), b"integrator"),
        ((scene, C.byref(params(background=2)), r, 4), b"background"),
    ]
    for args, word in cases:
        assert lib.vk_trace_radiance(*args, o, C.byref(st)) == ffi.VK_ERR_BAD_ARG, word
        assert word in lib.vk_last_error(), lib.vk_last_error()
        assert lib.vk_debug_trace_radiance_samples(*args, None, s, C.byref(st)) == ffi.VK_ERR_BAD_ARG, word
        assert word in lib.vk_last_error(), lib.vk_last_error()
    assert lib.vk_trace_radiance(scene, C.byref(rp), r, 4, None, C.byref(st)) == ffi.VK_ERR_BAD_ARG
    assert b"null rays or output" in lib.vk_last_error()
    assert lib.vk_debug_trace_radiance_samples(scene, C.byref(rp), r, 4, None, None, C.byref(st)) == ffi.VK_ERR_BAD_ARG
    # first_sample + samples_per_ray = 2^32 - 1 is the last window that is accepted (refused here for another reason only: flags)
    assert lib.vk_trace_radiance(scene, C.byref(params(samples_per_ray=4, first_sample=2 ** 32 - 5, flags=1)), r, 4, o, C.byref(st)) == \
        ffi.VK_ERR_BAD_ARG and b"flags" in lib.vk_last_error()
    # outputs untouched
    assert st.samples == 99 and (rgb == 7.0).all() and (samples == 7.0).all()
    # no rays: VK_OK, nothing done, also with null arrays (the scene handle is not read)
    assert lib.vk_trace_radiance(scene, C.byref(rp), None, 0, None, C.byref(st)) == ffi.VK_OK and st.samples == 0
    assert lib.vk_debug_trace_radiance_samples(scene, C.byref(rp), None, 0, None, None, None) == ffi.VK_OK


def test_the_kernel_is_new_and_has_its_instances(built):
    """radiance_kernel<F, MINW>: sphere-only worlds, Cornell-type worlds and everything, each with and without the PDF integrator —
    instances of their own, none of render_kernel's (whose budgets tests/test_kernel_resources.py pins)"""
    txt = open(build.kernel_resources_path()).read()
    seen = {}
    for blk in txt.split("Name: ")[1:]:
        m = re.search(r"radiance_kernelILj(\d+)ELi(\d+)E", blk.split("\n")[0])
        if m:
            get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
            seen[int(m.group(1))] = dict(minw=int(m.group(2)), vgprs=get("VGPRs"), agprs=get("AGPRs"), occupancy=get("Occupancy [waves/SIMD]"),
                                         static_lds=get("LDS Size [bytes/block]"), dynamic_stack="Dynamic Stack: True" in blk)
    cornell = 0x2 | 0x4 | 0x10 | 0x100
    assert set(seen) == {0, 0x80, cornell, cornell | 0x80, 0x17F, 0x17F | 0x80}, sorted(seen)
    for F, r in seen.items():
        assert r["occupancy"] >= r["minw"] and r["agprs"] == 0 and r["static_lds"] == 0 and not r["dynamic_stack"], (F, r)
        assert r["minw"] == (4 if F & 0x17F == 0x17F else 6), (F, r)
