"""Reconstruction filters (vk_splat_*, additive symbols of ABI 7) on the CPU: the seven functions and the three debug hooks declared,
exported by both libraries, bound, declared in the Rust shim; the two structs' sizes and offsets as gcc lays them out against the ctypes
mirror; no stream-taking function, no `void *`, and no name another family's pins would catch; the refusals that need no device, each
leaving its outputs untouched; the kernels of vk_splat.hip in a resource record of their own — exactly the new ones, without scratch,
AGPRs or a dynamic stack."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_splat_default_params", "vk_splat_create", "vk_splat_deposit", "vk_splat_resolve", "vk_splat_reset", "vk_splat_get_info",
             "vk_splat_destroy"]
HOOKS = ["vk_debug_splat_sums", "vk_debug_splat_form", "vk_debug_splat_last_ms"]
STRUCTS = {"vk_splat_params": ffi.SplatParams, "vk_splat_info": ffi.SplatInfo}
KERNELS = ["_Z20splat_deposit_kernelILb0EEv16SplatDepositArgs", "_Z20splat_deposit_kernelILb1EEv16SplatDepositArgs",
           "_Z20splat_resolve_kernel16SplatResolveArgs"]
FORBIDDEN = ("film", "paths", "regen", "adapt_", "roulette", "probe", "shade", "radiance")
TILED_LDS = 41616           # (256 + 4) x 5 pixels x 32 bytes, and the four waves' first anchors: as built


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
    assert lib.vk_splat_default_params.argtypes == [C.POINTER(ffi.SplatParams)]
    assert lib.vk_splat_create.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ffi.SplatParams), C.POINTER(C.c_void_p)]
    assert lib.vk_splat_deposit.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.vk_splat_resolve.argtypes == [C.c_void_p, C.c_void_p] and lib.vk_splat_reset.argtypes == [C.c_void_p]
    assert lib.vk_splat_get_info.argtypes == [C.c_void_p, C.POINTER(ffi.SplatInfo)]
    assert lib.vk_splat_destroy.restype is None and lib.vk_splat_destroy.argtypes == [C.c_void_p]
    assert lib.vk_debug_splat_sums.argtypes == [C.c_void_p, C.c_void_p] and lib.vk_debug_splat_form.argtypes == [C.c_void_p, C.c_uint32]
    assert lib.vk_debug_splat_last_ms.argtypes == [C.c_void_p, C.POINTER(C.c_double * 2)]
    assert all(getattr(lib, fn).restype is C.c_int for fn in FUNCTIONS[:-1] + HOOKS)
    assert (ffi.VK_SPLAT_BOX, ffi.VK_SPLAT_TENT, ffi.VK_SPLAT_MITCHELL) == (0, 1, 2)
    assert re.search(r"enum \{ VK_SPLAT_BOX = 0, VK_SPLAT_TENT = 1, VK_SPLAT_MITCHELL = 2 \};", code(hdr))
    assert (ffi.VK_DEBUG_SPLAT_FORM_DEFAULT, ffi.VK_DEBUG_SPLAT_FORM_PLAIN, ffi.VK_DEBUG_SPLAT_FORM_TILED) == (0, 1, 2)
    assert re.search(r"VK_DEBUG_SPLAT_FORM_DEFAULT = 0, VK_DEBUG_SPLAT_FORM_PLAIN = 1, VK_DEBUG_SPLAT_FORM_TILED = 2", header("vecchio_amd_debug.h"))
    sp = ffi.SplatParams(9, 9.0, 9.0, 9.0)
    assert lib.vk_splat_default_params(C.byref(sp)) == ffi.VK_OK
    third = np.float32(1.0) / np.float32(3.0)
    assert (sp.filter, sp.radius, sp.b, sp.c) == (ffi.VK_SPLAT_MITCHELL, 2.0, third, third)


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    want = {
        "vk_splat_default_params": r"out: \*mut vk_splat_params\) -> c_int;",
        "vk_splat_create": r"scene: \*mut vk_scene, width: u32, height: u32, samples_per_pixel: u32, sp: \*const vk_splat_params, "
                           r"out: \*mut \*mut vk_splat\) -> c_int;",
        "vk_splat_deposit": r"s: \*mut vk_splat, batch: \*mut vk_paths, positions: \*const f32\) -> c_int;",
        "vk_splat_resolve": r"s: \*mut vk_splat, rgb_out: \*mut f32\) -> c_int;",
        "vk_splat_reset": r"s: \*mut vk_splat\) -> c_int;",
        "vk_splat_get_info": r"s: \*mut vk_splat, out: \*mut vk_splat_info\) -> c_int;",
        "vk_splat_destroy": r"s: \*mut vk_splat\);",
    }
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    assert re.search(r"#\[repr\(C\)\] pub struct vk_splat \{ _private: \[u8; 0\] \}", rs)
    assert all(re.search(rf"pub const {n}: u32 = {v};", rs) for n, v in (("VK_SPLAT_BOX", 0), ("VK_SPLAT_TENT", 1), ("VK_SPLAT_MITCHELL", 2)))
    fields = {
        "vk_splat_params": "pub filter: u32, pub radius: f32, pub b: f32, pub c: f32",
        "vk_splat_info": "pub width: u32, pub height: u32, pub samples_per_pixel: u32, pub filter: u32, pub deposited: u64, pub dropped: u64, "
                         "pub clamped: u64, pub skipped: u64, pub deposits: u64, pub contributions: u64",
    }
    for name, f in fields.items():
        m = re.search(r"#\[repr\(C\)\][^{;]*?pub struct " + name + r"\s*\{(.*?)\}", rs, flags=re.S)
        assert m and " ".join(m.group(1).split()) == f, name
    import test_rust_shim_layout as R
    c, r = R.c_structs(), R.rust_structs()
    for name in fields:
        assert name in c and r.get(name) == c[name], name


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """vk_splat_params 16 bytes, vk_splat_info 64, and every field's offset and size: the header through gcc against ctypes"""
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
    assert seen["vk_splat_params"] == (16,) and seen["vk_splat_info"] == (64,)
    n = 0
    for cname, T in STRUCTS.items():
        assert C.sizeof(T) == seen[cname][0]
        for f, _ in T._fields_:
            d = getattr(T, f)
            assert seen[f"{cname}.{f}"] == (d.offset, d.size), (cname, f)
            n += 1
    assert n == 4 + 10
    assert [f for f, _ in ffi.SplatInfo._fields_] == ["width", "height", "samples_per_pixel", "filter", "deposited", "dropped", "clamped",
                                                      "skipped", "deposits", "contributions"]


def test_no_splat_function_takes_a_stream_and_no_other_pin_catches_one():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*splat\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args and "void *" not in args, fn
            assert not [w for w in FORBIDDEN if w in fn], fn
    assert seen == FUNCTIONS + HOOKS


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    h = C.c_void_p(0x1000)                # never read: each of these is refused first
    out = C.c_void_p(0x77)
    ok = ffi.SplatParams(ffi.VK_SPLAT_MITCHELL, 2.0, 0.5, 0.5)
    assert lib.vk_splat_default_params(None) == ffi.VK_ERR_BAD_ARG
    for args in ((None, 4, 4, 1, C.byref(ok), C.byref(out)), (h, 4, 4, 1, None, C.byref(out)), (h, 4, 4, 1, C.byref(ok), None)):
        assert lib.vk_splat_create(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    for dims, word in (((0, 4, 1), b"width and height must be >= 1"), ((4, 0, 1), b"width and height must be >= 1"),
                       ((8200, 8200, 1), b"width * height exceeds 2^26"), ((4, 4, 0), b"samples_per_pixel must be in 1..2^26"),
                       ((4, 4, (1 << 26) + 1), b"samples_per_pixel must be in 1..2^26")):
        assert lib.vk_splat_create(h, *dims, C.byref(ok), C.byref(out)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), dims
    nan, inf = float("nan"), float("inf")
    for fields, word in (((3, 1.0, 0.0, 0.0), b"unknown filter"), ((0xFFFFFFFF, 1.0, 0.0, 0.0), b"unknown filter"),
                         ((0, 0.49, 0.0, 0.0), b"radius must be finite and in [0.5, 2]"), ((1, 2.5, 0.0, 0.0), b"radius must be finite"),
                         ((1, nan, 0.0, 0.0), b"radius must be finite"), ((2, inf, 0.3, 0.3), b"radius must be finite"),
                         ((2, -1.0, 0.3, 0.3), b"radius must be finite"), ((2, 2.0, -0.1, 0.3), b"b and c must be finite and in [0, 1]"),
                         ((2, 2.0, 0.3, 1.5), b"b and c must be finite"), ((2, 2.0, nan, 0.3), b"b and c must be finite"),
                         ((2, 2.0, 0.3, inf), b"b and c must be finite")):
        bad = ffi.SplatParams(*fields)
        assert lib.vk_splat_create(h, 4, 4, 1, C.byref(bad), C.byref(out)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), fields
    assert out.value == 0x77
    pos = np.full(8, 7, np.float32)
    assert lib.vk_splat_deposit(None, h, None) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    assert lib.vk_splat_deposit(h, None, pos.ctypes.data) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    img = np.full(12, 7, np.float32)
    assert lib.vk_splat_resolve(None, img.ctypes.data) == ffi.VK_ERR_BAD_ARG and lib.vk_splat_resolve(h, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_splat_reset(None) == ffi.VK_ERR_BAD_ARG and b"null accumulator" in lib.vk_last_error()
    info = ffi.SplatInfo(9, 9, 9, 9, 9, 9, 9, 9, 9, 9)
    assert lib.vk_splat_get_info(None, C.byref(info)) == ffi.VK_ERR_BAD_ARG and lib.vk_splat_get_info(h, None) == ffi.VK_ERR_BAD_ARG
    assert bytes(info) == bytes(ffi.SplatInfo(9, 9, 9, 9, 9, 9, 9, 9, 9, 9))
    lib.vk_splat_destroy(None)            # nothing
    sums = np.full(8, 7, np.int64)
    assert lib.vk_debug_splat_sums(None, sums.ctypes.data) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_splat_sums(h, None) == ffi.VK_ERR_BAD_ARG
    ms = (C.c_double * 2)(7, 7)
    assert lib.vk_debug_splat_last_ms(None, C.byref(ms)) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_splat_last_ms(h, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_debug_splat_form(None, 0) == ffi.VK_ERR_BAD_ARG
    assert list(ms) == [7, 7] and (sums == 7).all() and (img == 7).all() and (pos == 7).all()


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
    """kernel_resources_splat.txt lists exactly the kernels of vk_splat.hip, each once: no scratch, no AGPRs, no dynamic stack; LDS in
    the TILED form only, of the size it was built with (three workgroups a CU), the others at full occupancy; no name another pin would
    catch, the argument structs' types included; kernel_resources.txt and kernel_resources_adapt.txt hold none of them"""
    mine = resources(build.kernel_resources_splat_path())
    assert sorted(mine) == sorted(KERNELS), sorted(mine)
    for name, r in mine.items():
        assert not [w for w in FORBIDDEN if w in name.lower()], name
        assert r["agprs"] == 0 and r["scratch"] == 0 and r["scratch_ops"] == 0 and not r["dynamic_stack"], (name, r)
        tiled = "ILb1E" in name
        assert r["lds"] == (TILED_LDS if tiled else 0), (name, r)
        assert r["occupancy"] == (3 if tiled else 8), (name, r)
    for path in (build.kernel_resources_path(), build.kernel_resources_adapt_path()):
        assert not [n for n in resources(path) if "splat" in n.lower()] and "splat" not in open(path).read().lower()
    src = open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_splat.h")).read()
    assert re.search(r"constexpr bool SPLAT_DEFAULT_TILED = (true|false);", src)      # the measured default
