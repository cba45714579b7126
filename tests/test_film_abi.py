"""Films (vk_film_*, additive symbols of ABI 7) on the CPU: the seven functions and the three debug hooks declared, exported by both
libraries, bound, declared in the Rust shim; the two structs' sizes and offsets as gcc lays them out against the ctypes mirror; no
stream-taking function and no `void *`; no name a path batch's pins would catch; the refusals that need no device; the new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_film_create", "vk_film_emit", "vk_film_deposit", "vk_film_resolve", "vk_film_reset", "vk_film_get_info", "vk_film_destroy"]
HOOKS = ["vk_debug_film_sums", "vk_debug_film_last_ms", "vk_debug_film_deposit_form"]
STRUCTS = {"vk_film_window": ffi.FilmWindow, "vk_film_info": ffi.FilmInfo}


def header(name="vecchio_amd.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_declared_exported_and_bound(built):
    hdr = header()
    assert re.search(r"#define VK_ABI_VERSION 7\b", hdr)
    for fn in FUNCTIONS:
        assert re.search(r"\b(?:int|void)\s+" + fn + r"\s*\(", code(hdr)), fn
        assert fn in ffi.DEVICE_SYMBOLS, fn
    for fn in HOOKS:
        assert re.search(r"\bint " + fn + r"\s*\(", code(header("vecchio_amd_debug.h"))), fn
    for path in (ffi.device_lib_path(), build.build_device_debug()):
        lib = C.CDLL(path)
        for fn in FUNCTIONS + HOOKS:
            assert hasattr(lib, fn), (path, fn)
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == 7
    assert lib.vk_film_create.argtypes == [C.c_void_p, C.POINTER(ffi.Camera), C.POINTER(ffi.RenderParams), C.POINTER(C.c_void_p)]
    assert lib.vk_film_emit.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(ffi.FilmWindow)]
    assert lib.vk_film_deposit.argtypes == [C.c_void_p, C.c_void_p]
    assert lib.vk_film_resolve.argtypes == [C.c_void_p, C.c_uint32, C.c_void_p]
    assert lib.vk_film_reset.argtypes == [C.c_void_p, C.POINTER(ffi.Camera)]
    assert lib.vk_film_get_info.argtypes == [C.c_void_p, C.POINTER(ffi.FilmInfo)]
    assert lib.vk_film_destroy.restype is None and lib.vk_film_emit.restype is C.c_int
    assert (ffi.VK_DEBUG_FILM_DEPOSIT_PLAIN, ffi.VK_DEBUG_FILM_DEPOSIT_RUNS) == (0, 1)
    assert re.search(r"VK_DEBUG_FILM_DEPOSIT_PLAIN = 0, VK_DEBUG_FILM_DEPOSIT_RUNS = 1", header("vecchio_amd_debug.h"))


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    want = {
        "vk_film_create": r"scene: \*mut vk_scene, cam: \*const vk_camera, params: \*const vk_render_params, out: \*mut \*mut vk_film\) -> c_int;",
        "vk_film_emit": r"film: \*mut vk_film, batch: \*mut vk_paths, win: \*const vk_film_window\) -> c_int;",
        "vk_film_deposit": r"film: \*mut vk_film, batch: \*mut vk_paths\) -> c_int;",
        "vk_film_resolve": r"film: \*mut vk_film, n: u32, rgb_out: \*mut f32\) -> c_int;",
        "vk_film_reset": r"film: \*mut vk_film, cam: \*const vk_camera\) -> c_int;",
        "vk_film_get_info": r"film: \*mut vk_film, out: \*mut vk_film_info\) -> c_int;",
        "vk_film_destroy": r"film: \*mut vk_film\);",
    }
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    assert re.search(r"#\[repr\(C\)\] pub struct vk_film \{ _private: \[u8; 0\] \}", rs)
    fields = {
        "vk_film_window": "pub x0: u32, pub y0: u32, pub width: u32, pub height: u32, pub first_sample: u32, pub n_samples: u32",
        "vk_film_info": "pub width: u32, pub height: u32, pub samples_per_pixel: u32, pub _pad: u32, pub emitted: u64, pub deposited: u64, "
                        "pub dropped: u64, pub clamped: u64, pub skipped: u64, pub deposits: u64",
    }
    for name, f in fields.items():
        m = re.search(r"#\[repr\(C\)\][^{;]*?pub struct " + name + r"\s*\{(.*?)\}", rs, flags=re.S)
        assert m and " ".join(m.group(1).split()) == f, name


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """vk_film_window 24 bytes, vk_film_info 64, and every field's offset and size: the header through gcc against ctypes"""
    lines = []
    for cname, T in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
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
    assert seen["vk_film_window"] == (24,) and seen["vk_film_info"] == (64,)
    n = 0
    for cname, T in STRUCTS.items():
        assert C.sizeof(T) == seen[cname][0]
        for f, _ in T._fields_:
            d = getattr(T, f)
            assert seen[f"{cname}.{f}"] == (d.offset, d.size), (cname, f)
            n += 1
    assert n == 6 + 10


def test_no_film_function_takes_a_stream_or_a_void_pointer():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*film\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args and "void *" not in args, fn
            assert "paths" not in fn, fn                   # (tests/test_paths_abi.py pins the functions with that word)
    assert seen == FUNCTIONS + HOOKS


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    film = C.c_void_p(0x1000)             # never read: each of these is refused first
    h = C.c_void_p(0x77)
    cam, p = ffi.Camera(), ffi.RenderParams()
    assert lib.vk_film_create(film, C.byref(cam), C.byref(p), None) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    for args in ((None, C.byref(cam), C.byref(p)), (film, None, C.byref(p)), (film, C.byref(cam), None)):
        assert lib.vk_film_create(*args, C.byref(h)) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    assert h.value == 0x77
    win = ffi.FilmWindow(0, 0, 4, 4, 0, 1)
    assert lib.vk_film_emit(None, film, C.byref(win)) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    assert lib.vk_film_emit(film, None, C.byref(win)) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_film_emit(film, film, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_film_deposit(None, film) == ffi.VK_ERR_BAD_ARG and lib.vk_film_deposit(film, None) == ffi.VK_ERR_BAD_ARG
    img = np.full(12, 7, np.float32)
    assert lib.vk_film_resolve(None, 1, img.ctypes.data) == ffi.VK_ERR_BAD_ARG and lib.vk_film_resolve(film, 1, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_film_resolve(film, 0, img.ctypes.data) == ffi.VK_ERR_BAD_ARG and b"n must be >= 1" in lib.vk_last_error()
    assert lib.vk_film_reset(None, None) == ffi.VK_ERR_BAD_ARG and b"null film" in lib.vk_last_error()
    info = ffi.FilmInfo()
    info.emitted = 99
    assert lib.vk_film_get_info(None, C.byref(info)) == ffi.VK_ERR_BAD_ARG and lib.vk_film_get_info(film, None) == ffi.VK_ERR_BAD_ARG
    assert info.emitted == 99 and (img == 7).all()
    lib.vk_film_destroy(None)             # nothing
    sums = np.full(6, 7, np.int64)
    assert lib.vk_debug_film_sums(None, sums.ctypes.data) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_film_sums(film, None) == ffi.VK_ERR_BAD_ARG
    ms = (C.c_double * 3)(7, 7, 7)
    assert lib.vk_debug_film_last_ms(None, C.byref(ms)) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_film_last_ms(film, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_debug_film_deposit_form(None, 0) == ffi.VK_ERR_BAD_ARG
    assert list(ms) == [7, 7, 7] and (sums == 7).all()


def test_the_kernels_are_new(built):
    """film_emit_kernel and film_deposit_kernel in its forms: no AGPRs, no scratch, no dynamic stack, no LDS; and no name the path
    batch's kernel pin (tests/test_paths_abi.py: `paths_` in the mangled name, a by-value argument struct's type included) would catch"""
    txt = open(build.kernel_resources_path()).read()
    src = open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_kernels.h")).read()
    seen = {}
    for blk in txt.split("Name: ")[1:]:
        name = blk.split("\n")[0]
        if "film_" not in name:
            continue
        get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
        assert name not in seen
        seen[name] = dict(vgprs=get("VGPRs"), agprs=get("AGPRs"), scratch=get("ScratchSize [bytes/lane]"), scratch_ops=get("ScratchOps"),
                          occupancy=get("Occupancy [waves/SIMD]"), lds=get("LDS Size [bytes/block]"), dynamic_stack="Dynamic Stack: True" in blk)
    assert sum("film_emit_kernel" in k for k in seen) == 1, sorted(seen)
    forms = sorted(re.search(r"film_deposit_kernelILb([01])EE", k).group(1) for k in seen if "film_deposit_kernel" in k)
    assert forms == ["0", "1"], forms                     # PLAIN and RUNS
    assert len(seen) == 3, sorted(seen)
    assert re.search(r"constexpr bool FILM_DEPOSIT_RUNS = true;", src)          # the measured default (DESIGN.md "Film")
    for name, r in seen.items():
        assert "paths_" not in name, name
        assert r["agprs"] == 0 and r["scratch"] == 0 and r["scratch_ops"] == 0 and not r["dynamic_stack"] and r["lds"] == 0, (name, r)
        assert r["occupancy"] >= 8, (name, r)
