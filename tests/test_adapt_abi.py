"""A film's error moments and adaptive regeneration (vk_adapt_*, additive symbols of ABI 7) on the CPU: the six functions and the three
debug hooks declared, exported by both libraries, bound, declared in the Rust shim; vk_adapt_info's size and offsets as gcc lays them
out against the ctypes mirror; no stream-taking function, and no name the film's, the regeneration's or the path batch's pins would
catch; the refusals that need no device, each leaving its outputs untouched; the kernels of vk_adapt.hip in a resource record of their
own — exactly the new ones, without scratch, AGPRs or a dynamic stack, at full occupancy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_adapt_enable", "vk_adapt_begin", "vk_adapt_close", "vk_adapt_resolve", "vk_adapt_stderr", "vk_adapt_tile_samples"]
HOOKS = ["vk_debug_adapt_moments", "vk_debug_adapt_set_tiles", "vk_debug_adapt_sequence"]
KERNELS = ["adapt_emit_kernel", "adapt_sequence_kernel", "adapt_close_kernel", "adapt_count_kernel", "adapt_scatter_kernel",
           "adapt_resolve_kernel", "adapt_stderr_kernel"]


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
    assert lib.vk_adapt_enable.argtypes == [C.c_void_p, C.POINTER(ffi.AdaptiveParams)]
    assert lib.vk_adapt_begin.argtypes == [C.c_void_p, C.c_void_p, C.c_uint32]
    assert lib.vk_adapt_close.argtypes == [C.c_void_p, C.c_uint32, C.POINTER(ffi.AdaptInfo)]
    assert lib.vk_adapt_resolve.argtypes == [C.c_void_p, C.c_void_p] and lib.vk_adapt_stderr.argtypes == [C.c_void_p, C.c_void_p]
    assert lib.vk_adapt_tile_samples.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(ffi.AdaptiveInfo)]
    assert lib.vk_debug_adapt_sequence.argtypes == [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    assert all(getattr(lib, fn).restype is C.c_int for fn in FUNCTIONS + HOOKS)


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    want = {
        "vk_adapt_enable": r"film: \*mut vk_film, ap: \*const vk_adaptive_params\) -> c_int;",
        "vk_adapt_begin": r"film: \*mut vk_film, batch: \*mut vk_paths, n_samples: u32\) -> c_int;",
        "vk_adapt_close": r"film: \*mut vk_film, n_samples: u32, info: \*mut vk_adapt_info\) -> c_int;",
        "vk_adapt_resolve": r"film: \*mut vk_film, rgb_out: \*mut f32\) -> c_int;",
        "vk_adapt_stderr": r"film: \*mut vk_film, out: \*mut f32\) -> c_int;",
        "vk_adapt_tile_samples": r"film: \*mut vk_film, out: \*mut u32, info: \*mut vk_adaptive_info\) -> c_int;",
    }
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    m = re.search(r"#\[repr\(C\)\][^{;]*?pub struct vk_adapt_info\s*\{(.*?)\}", rs, flags=re.S)
    assert m and " ".join(m.group(1).split()) == (
        "pub samples_done: u32, pub steps: u32, pub tiles_total: u32, pub tiles_active: u32, pub pixels_active: u64, "
        "pub samples_rendered: u64")
    import test_rust_shim_layout as R
    c, r = R.c_structs(), R.rust_structs()
    assert "vk_adapt_info" in c and r.get("vk_adapt_info") == c["vk_adapt_info"]


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """vk_adapt_info is 32 bytes, and every field's offset and size: the header through gcc against ctypes"""
    T, cname = ffi.AdaptInfo, "vk_adapt_info"
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
    assert seen[cname] == (32,) and C.sizeof(T) == 32
    for f, _ in T._fields_:
        d = getattr(T, f)
        assert seen[f"{cname}.{f}"] == (d.offset, d.size), f
    assert [f for f, _ in T._fields_] == ["samples_done", "steps", "tiles_total", "tiles_active", "pixels_active", "samples_rendered"]


def test_no_adapt_function_takes_a_stream_and_no_other_pin_catches_one():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*adapt_\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args and "void *" not in args, fn
            assert "film" not in fn and "regen" not in fn and "paths" not in fn, fn
    assert seen == FUNCTIONS + HOOKS


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    h = C.c_void_p(0x1000)                # never read: each of these is refused first
    ok = ffi.AdaptiveParams(1e-3, 0.0, 0, 2)
    assert lib.vk_adapt_enable(None, C.byref(ok)) == ffi.VK_ERR_BAD_ARG and b"null film" in lib.vk_last_error()
    assert lib.vk_adapt_enable(None, None) == ffi.VK_ERR_BAD_ARG and b"null film" in lib.vk_last_error()
    # the parameters are checked in vk_progress_set_adaptive's words, before the film is read
    for fields, word in (((1e-3, 0.0, 0, 1), b"min_steps must be >= 2"), ((1e-3, 0.0, 0, 0), b"min_steps must be >= 2"),
                         ((-1.0, 0.0, 0, 2), b"finite and >= 0"), ((0.0, -1e-9, 0, 2), b"finite and >= 0"),
                         ((float("nan"), 0.0, 0, 2), b"finite and >= 0"), ((0.0, float("inf"), 0, 2), b"finite and >= 0")):
        bad = ffi.AdaptiveParams(*fields)
        assert lib.vk_adapt_enable(h, C.byref(bad)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), fields
    assert lib.vk_adapt_begin(None, h, 1) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    assert lib.vk_adapt_begin(h, None, 1) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    info = ffi.AdaptInfo(9, 9, 9, 9, 9, 9)
    assert lib.vk_adapt_close(None, 1, C.byref(info)) == ffi.VK_ERR_BAD_ARG and b"null film" in lib.vk_last_error()
    assert bytes(info) == bytes(ffi.AdaptInfo(9, 9, 9, 9, 9, 9))
    img = np.full(12, 7, np.float32)
    assert lib.vk_adapt_resolve(None, img.ctypes.data) == ffi.VK_ERR_BAD_ARG and lib.vk_adapt_resolve(h, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_adapt_stderr(None, img.ctypes.data) == ffi.VK_ERR_BAD_ARG and lib.vk_adapt_stderr(h, None) == ffi.VK_ERR_BAD_ARG
    tiles, ainfo = np.full(4, 7, np.uint32), ffi.AdaptiveInfo(9, 9, 9)
    assert lib.vk_adapt_tile_samples(None, tiles.ctypes.data, C.byref(ainfo)) == ffi.VK_ERR_BAD_ARG
    assert bytes(ainfo) == bytes(ffi.AdaptiveInfo(9, 9, 9))
    run, m2 = np.full(6, 7, np.int64), np.full(6, 7.0)
    assert lib.vk_debug_adapt_moments(None, run.ctypes.data, m2.ctypes.data) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_debug_adapt_set_tiles(None, tiles.ctypes.data, tiles.ctypes.data) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_debug_adapt_set_tiles(h, None, tiles.ctypes.data) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_debug_adapt_set_tiles(h, tiles.ctypes.data, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_debug_adapt_sequence(None, 1, 0, 4, tiles.ctypes.data, tiles.ctypes.data) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_debug_adapt_sequence(h, 1, 0, 4, None, tiles.ctypes.data) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_debug_adapt_sequence(h, 1, 0, 4, tiles.ctypes.data, None) == ffi.VK_ERR_BAD_ARG
    assert (img == 7).all() and (tiles == 7).all() and (run == 7).all() and (m2 == 7).all()


def resources(path):
    out = {}
    for blk in open(path).read().split("Name: ")[1:]:
        name = blk.split("\n")[0].strip()
        assert name not in out
        get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
        out[name] = dict(vgprs=get("VGPRs"), agprs=get("AGPRs"), scratch=get("ScratchSize [bytes/lane]"), scratch_ops=get("ScratchOps"),
                         occupancy=get("Occupancy [waves/SIMD]"), lds=get("LDS Size [bytes/block]"), dynamic_stack="Dynamic Stack: True" in blk)
    return out


def test_the_kernels_are_new_and_in_a_record_of_their_own(built):
    """kernel_resources_adapt.txt lists exactly the kernels of vk_adapt.hip, each once: no scratch, no AGPRs, no dynamic stack,
    occupancy >= 8; no name another pin would catch (`film_`, `regen` or `paths_` in the mangled name, the argument struct's type
    included); and kernel_resources.txt, which tests/test_roulette_abi.py pins, holds none of them"""
    mine = resources(build.kernel_resources_adapt_path())
    assert len(mine) == len(KERNELS), sorted(mine)
    for k in KERNELS:
        names = [n for n in mine if re.fullmatch(r"_Z\d+" + k + r"\d+Adapt\w+Args", n)]
        assert len(names) == 1, (k, sorted(mine))
    for name, r in mine.items():
        assert "film_" not in name and "paths_" not in name and "regen" not in name.lower(), name
        assert r["agprs"] == 0 and r["scratch"] == 0 and r["scratch_ops"] == 0 and not r["dynamic_stack"], (name, r)
        assert r["occupancy"] >= 8, (name, r)
    assert not [n for n in resources(build.kernel_resources_path()) if "adapt_" in n]
