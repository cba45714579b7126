"""Regeneration (vk_regen_*, additive symbols of ABI 7) on the CPU: the three functions and the debug hook declared, exported by both
libraries, bound, declared in the Rust shim; vk_regen_info's size and offsets as gcc lays them out against the ctypes mirror; no
stream-taking function and no `void *`; no name the film's or the path batch's pins would catch; the refusals that need no device; the
two new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_regen_begin", "vk_regen_step", "vk_regen_cull"]
HOOKS = ["vk_debug_regen_last_ms"]


def header(name="vecchio_amd.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_declared_exported_and_bound(built):
    hdr = header()
    assert re.search(r"#define VK_ABI_VERSION 7\b", hdr)
    for fn in FUNCTIONS:
        assert re.search(r"\bint\s+" + fn + r"\s*\(", code(hdr)), fn
        assert fn in ffi.DEVICE_SYMBOLS, fn
    for fn in HOOKS:
        assert re.search(r"\bint " + fn + r"\s*\(", code(header("vecchio_amd_debug.h"))), fn
    for path in (ffi.device_lib_path(), build.build_device_debug()):
        lib = C.CDLL(path)
        for fn in FUNCTIONS + HOOKS:
            assert hasattr(lib, fn), (path, fn)
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == 7
    assert lib.vk_regen_begin.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(ffi.FilmWindow)]
    assert lib.vk_regen_step.argtypes == [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ffi.RegenInfo)]
    assert lib.vk_regen_cull.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.vk_debug_regen_last_ms.argtypes == [C.c_void_p, C.POINTER(C.c_double * 4)]
    assert all(getattr(lib, fn).restype is C.c_int for fn in FUNCTIONS + HOOKS)


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    want = {
        "vk_regen_begin": r"film: \*mut vk_film, batch: \*mut vk_paths, win: \*const vk_film_window\) -> c_int;",
        "vk_regen_step": r"film: \*mut vk_film, batch: \*mut vk_paths, max_bounces: u32, info: \*mut vk_regen_info\) -> c_int;",
        "vk_regen_cull": r"film: \*mut vk_film, batch: \*mut vk_paths, keep: \*const u8, scale: \*const f32\) -> c_int;",
    }
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    m = re.search(r"#\[repr\(C\)\][^{;]*?pub struct vk_regen_info\s*\{(.*?)\}", rs, flags=re.S)
    assert m and " ".join(m.group(1).split()) == (
        "pub traced: u64, pub live: u64, pub remaining: u64, pub emitted: u64, pub missed: u64, pub ended: u64, pub bad: u64, "
        "pub bounces: u32, pub kernel_launches: u32, pub kernel_ms: f64, pub seconds: f64")


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """vk_regen_info is 80 bytes, and every field's offset and size: the header through gcc against ctypes"""
    T, cname = ffi.RegenInfo, "vk_regen_info"
    lines = [f'printf("{cname} %zu\\n", sizeof({cname}));']
    for f, _ in T._fields_:
        lines.append(f'printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname} *)0)->{f}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vecchio_amd.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    seen = {}
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if ln:
            k, *v = ln.split()
            seen[k] = tuple(int(x) for x in v)
    assert seen[cname] == (80,) and C.sizeof(T) == 80
    for f, _ in T._fields_:
        d = getattr(T, f)
        assert seen[f"{cname}.{f}"] == (d.offset, d.size), f
    assert [f for f, _ in T._fields_] == ["traced", "live", "remaining", "emitted", "missed", "ended", "bad", "bounces", "kernel_launches",
                                          "kernel_ms", "seconds"]


def test_no_regen_function_takes_a_stream_or_a_void_pointer_or_a_pinned_word():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*regen\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args and "void *" not in args, fn
            assert "film" not in fn and "paths" not in fn, fn        # (tests/test_film_abi.py and tests/test_paths_abi.py pin those)
    assert seen == FUNCTIONS + HOOKS


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    h = C.c_void_p(0x1000)                # never read: each of these is refused first
    win = ffi.FilmWindow(0, 0, 4, 4, 0, 1)
    for args in ((None, h, C.byref(win)), (h, None, C.byref(win)), (h, h, None)):
        assert lib.vk_regen_begin(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    info = ffi.RegenInfo()
    info.traced = info.remaining = 99
    assert lib.vk_regen_step(None, h, 1, C.byref(info)) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    assert lib.vk_regen_step(h, None, 1, C.byref(info)) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    assert info.traced == 99 and info.remaining == 99
    keep = np.ones(4, np.uint8)
    assert lib.vk_regen_cull(None, h, keep.ctypes.data, None) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    assert lib.vk_regen_cull(h, None, keep.ctypes.data, None) == ffi.VK_ERR_BAD_ARG
    ms = (C.c_double * 4)(7, 7, 7, 7)
    assert lib.vk_debug_regen_last_ms(None, C.byref(ms)) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_regen_last_ms(h, None) == ffi.VK_ERR_BAD_ARG
    assert list(ms) == [7, 7, 7, 7]


def test_the_kernels_are_new(built):
    """regen_move_kernel and regen_emit_kernel: no AGPRs, no scratch, no dynamic stack, LDS in the move pass only; and no name the
    film's or the path batch's kernel pins would catch (`film_` or `paths_` in the mangled name, a by-value argument struct's type
    included)"""
    txt = open(build.kernel_resources_path()).read()
    seen = {}
    for blk in txt.split("Name: ")[1:]:
        name = blk.split("\n")[0]
        if "regen" not in name.lower():
            continue
        get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
        assert name not in seen
        seen[name] = dict(vgprs=get("VGPRs"), agprs=get("AGPRs"), scratch=get("ScratchSize [bytes/lane]"), scratch_ops=get("ScratchOps"),
                          occupancy=get("Occupancy [waves/SIMD]"), lds=get("LDS Size [bytes/block]"), dynamic_stack="Dynamic Stack: True" in blk)
    assert sum("regen_move_kernel" in k for k in seen) == 1 and sum("regen_emit_kernel" in k for k in seen) == 1, sorted(seen)
    assert len(seen) == 2, sorted(seen)
    for name, r in seen.items():
        assert "film_" not in name and "paths_" not in name, name
        assert r["agprs"] == 0 and r["scratch"] == 0 and r["scratch_ops"] == 0 and not r["dynamic_stack"], (name, r)
        assert (r["lds"] > 0) == ("regen_move_kernel" in name) and r["lds"] <= 256, (name, r)
        assert r["occupancy"] >= 8, (name, r)
