"""Robust film (vk_robust_*, additive symbols of ABI 7) on the CPU: the seven functions and the two debug hooks declared, exported by
both libraries, bound, declared in the Rust shim; the two structs' sizes and offsets as gcc lays them out against the ctypes mirror; no
stream-taking function; the refusals that need no device, each leaving its outputs untouched; the kernels of vk_robust.hip in a
resource record of their own — exactly the new ones, without scratch, AGPRs, LDS or a dynamic stack — and in none of the other four."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_robust_default_params", "vk_robust_create", "vk_robust_deposit", "vk_robust_resolve", "vk_robust_reset",
             "vk_robust_get_info", "vk_robust_destroy"]
HOOKS = ["vk_debug_robust_sums", "vk_debug_robust_last_ms"]
STRUCTS = {"vk_robust_params": ffi.RobustParams, "vk_robust_info": ffi.RobustInfo}
KERNELS = ["_Z21robust_deposit_kernel17RobustDepositArgs"] + [f"_Z21robust_resolve_kernelILi{k}EEv17RobustResolveArgs" for k in range(2, 17)]


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
    assert lib.vk_robust_default_params.argtypes == [C.POINTER(ffi.RobustParams)]
    assert lib.vk_robust_create.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ffi.RobustParams), C.POINTER(C.c_void_p)]
    assert lib.vk_robust_deposit.argtypes == [C.c_void_p, C.c_void_p]
    assert lib.vk_robust_resolve.argtypes == [C.c_void_p, C.POINTER(ffi.RobustParams), C.c_void_p, C.c_void_p]
    assert lib.vk_robust_reset.argtypes == [C.c_void_p] and lib.vk_robust_get_info.argtypes == [C.c_void_p, C.POINTER(ffi.RobustInfo)]
    assert lib.vk_robust_destroy.restype is None and lib.vk_robust_destroy.argtypes == [C.c_void_p]
    assert lib.vk_debug_robust_sums.argtypes == [C.c_void_p, C.c_void_p]
    assert lib.vk_debug_robust_last_ms.argtypes == [C.c_void_p, C.POINTER(C.c_double * 2)]
    assert all(getattr(lib, fn).restype is C.c_int for fn in FUNCTIONS[:-1] + HOOKS)
    assert (ffi.VK_ROBUST_MEAN, ffi.VK_ROBUST_TRIM, ffi.VK_ROBUST_GINI) == (0, 1, 2)
    assert re.search(r"enum \{ VK_ROBUST_MEAN = 0, VK_ROBUST_TRIM = 1, VK_ROBUST_GINI = 2 \};", code(hdr))
    rp = ffi.RobustParams(9, 9, 9, 9)
    assert lib.vk_robust_default_params(C.byref(rp)) == ffi.VK_OK
    assert (rp.buckets, rp.mode, rp.trim, rp._pad) == (8, ffi.VK_ROBUST_GINI, 0, 0)


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    want = {
        "vk_robust_default_params": r"out: \*mut vk_robust_params\) -> c_int;",
        "vk_robust_create": r"scene: \*mut vk_scene, width: u32, height: u32, samples_per_pixel: u32, rp: \*const vk_robust_params, "
                            r"out: \*mut \*mut vk_robust\) -> c_int;",
        "vk_robust_deposit": r"s: \*mut vk_robust, batch: \*mut vk_paths\) -> c_int;",
        "vk_robust_resolve": r"s: \*mut vk_robust, how: \*const vk_robust_params, rgb_out: \*mut f32, stderr3_out: \*mut f32\) -> c_int;",
        "vk_robust_reset": r"s: \*mut vk_robust\) -> c_int;",
        "vk_robust_get_info": r"s: \*mut vk_robust, out: \*mut vk_robust_info\) -> c_int;",
        "vk_robust_destroy": r"s: \*mut vk_robust\);",
    }
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    assert re.search(r"#\[repr\(C\)\] pub struct vk_robust \{ _private: \[u8; 0\] \}", rs)
    assert all(re.search(rf"pub const {n}: u32 = {v};", rs) for n, v in (("VK_ROBUST_MEAN", 0), ("VK_ROBUST_TRIM", 1), ("VK_ROBUST_GINI", 2)))
    fields = {
        "vk_robust_params": "pub buckets: u32, pub mode: u32, pub trim: u32, pub _pad: u32",
        "vk_robust_info": "pub width: u32, pub height: u32, pub samples_per_pixel: u32, pub buckets: u32, pub deposited: u64, "
                          "pub dropped: u64, pub clamped: u64, pub skipped: u64, pub deposits: u64, pub _reserved: u64",
    }
    for name, f in fields.items():
        m = re.search(r"#\[repr\(C\)\][^{;]*?pub struct " + name + r"\s*\{(.*?)\}", rs, flags=re.S)
        assert m and " ".join(m.group(1).split()) == f, name
    import test_rust_shim_layout as R
    c, r = R.c_structs(), R.rust_structs()
    for name in fields:
        assert name in c and r.get(name) == c[name], name


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """vk_robust_params 16 bytes, vk_robust_info 64, and every field's offset and size: the header through gcc against ctypes"""
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
    assert seen["vk_robust_params"] == (16,) and seen["vk_robust_info"] == (64,)
    n = 0
    for cname, T in STRUCTS.items():
        assert C.sizeof(T) == seen[cname][0]
        for f, _ in T._fields_:
            d = getattr(T, f)
            assert seen[f"{cname}.{f}"] == (d.offset, d.size), (cname, f)
            n += 1
    assert n == 4 + 10
    assert [f for f, _ in ffi.RobustParams._fields_] == ["buckets", "mode", "trim", "_pad"]
    assert [f for f, _ in ffi.RobustInfo._fields_] == ["width", "height", "samples_per_pixel", "buckets", "deposited", "dropped", "clamped",
                                                       "skipped", "deposits", "_reserved"]


def test_no_robust_function_takes_a_stream():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*robust\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args and "void *" not in args and "_device" not in fn, fn
    assert seen == FUNCTIONS + HOOKS


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    h = C.c_void_p(0x1000)                # never read: each of these is refused first
    out = C.c_void_p(0x77)
    ok = ffi.RobustParams(8, ffi.VK_ROBUST_GINI, 0, 0)
    assert lib.vk_robust_default_params(None) == ffi.VK_ERR_BAD_ARG
    for args in ((None, 4, 4, 1, C.byref(ok), C.byref(out)), (h, 4, 4, 1, None, C.byref(out)), (h, 4, 4, 1, C.byref(ok), None)):
        assert lib.vk_robust_create(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    for dims, word in (((0, 4, 1), b"width and height must be >= 1"), ((4, 0, 1), b"width and height must be >= 1"),
                       ((4097, 4096, 1), b"width * height * buckets exceeds 2^27"), ((0xFFFFFFFF, 0xFFFFFFFF, 1), b"exceeds 2^27"),
                       ((4, 4, 0), b"samples_per_pixel must be in 1..2^26"), ((4, 4, (1 << 26) + 1), b"samples_per_pixel must be in 1..2^26")):
        assert lib.vk_robust_create(h, *dims, C.byref(ok), C.byref(out)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), dims
    for fields, word in (((1, 0, 0, 0), b"buckets must be in 2..16"), ((0, 0, 0, 0), b"buckets must be in 2..16"),
                         ((17, 2, 0, 0), b"buckets must be in 2..16"), ((8, 3, 0, 0), b"unknown mode"), ((8, 0xFFFFFFFF, 0, 0), b"unknown mode"),
                         ((8, 2, 0, 1), b"_pad must be 0")):
        bad = ffi.RobustParams(*fields)
        assert lib.vk_robust_create(h, 4, 4, 1, C.byref(bad), C.byref(out)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), fields
    # 4096 x 4096 x 8 is 2^27 exactly: admitted as far as the arguments go (16 buckets are not)
    big = ffi.RobustParams(16, 0, 0, 0)
    assert lib.vk_robust_create(h, 4096, 4096, 1, C.byref(big), C.byref(out)) == ffi.VK_ERR_BAD_ARG and b"exceeds 2^27" in lib.vk_last_error()
    assert out.value == 0x77
    assert lib.vk_robust_deposit(None, h) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    assert lib.vk_robust_deposit(h, None) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    img, se = np.full(12, 7, np.float32), np.full(12, 7, np.float32)
    assert lib.vk_robust_resolve(None, None, img.ctypes.data, se.ctypes.data) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_robust_resolve(h, None, None, se.ctypes.data) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    assert lib.vk_robust_reset(None) == ffi.VK_ERR_BAD_ARG and b"null accumulator" in lib.vk_last_error()
    info = ffi.RobustInfo(9, 9, 9, 9, 9, 9, 9, 9, 9, 9)
    assert lib.vk_robust_get_info(None, C.byref(info)) == ffi.VK_ERR_BAD_ARG and lib.vk_robust_get_info(h, None) == ffi.VK_ERR_BAD_ARG
    assert bytes(info) == bytes(ffi.RobustInfo(9, 9, 9, 9, 9, 9, 9, 9, 9, 9))
    lib.vk_robust_destroy(None)           # nothing
    sums = np.full(8, 7, np.int64)
    assert lib.vk_debug_robust_sums(None, sums.ctypes.data) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_robust_sums(h, None) == ffi.VK_ERR_BAD_ARG
    ms = (C.c_double * 2)(7, 7)
    assert lib.vk_debug_robust_last_ms(None, C.byref(ms)) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_robust_last_ms(h, None) == ffi.VK_ERR_BAD_ARG
    assert list(ms) == [7, 7] and (sums == 7).all() and (img == 7).all() and (se == 7).all()


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
    """kernel_resources_robust.txt lists exactly the kernels of vk_robust.hip, each once — the deposit and one resolve per K in 2..16 —:
    no scratch (the K-bucket table stays in registers for every K), no AGPRs, no LDS (there is no merging form), no dynamic stack;
    the other four records hold none of them"""
    mine = resources(build.kernel_resources_robust_path())
    assert sorted(mine) == sorted(KERNELS), sorted(mine)
    for name, r in mine.items():
        assert r["agprs"] == 0 and r["scratch"] == 0 and r["scratch_ops"] == 0 and not r["dynamic_stack"] and r["lds"] == 0, (name, r)
        assert r["vgprs"] <= 256, (name, r)
    assert mine[KERNELS[0]]["occupancy"] == 8
    for path in (build.kernel_resources_path(), build.kernel_resources_adapt_path(), build.kernel_resources_splat_path(),
                 build.kernel_resources_matte_path()):
        assert not [n for n in resources(path) if "robust" in n.lower()] and "robust" not in open(path).read().lower(), path
    src = open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_robust.hip")).read()
    assert len(re.findall(r"__global__", src)) == 2 and "__shared__" not in src
