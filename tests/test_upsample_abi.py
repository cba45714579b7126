"""Guided upsampling (vk_upsample_*, additive symbols of ABI 7) on the CPU: the nine functions and the two debug hooks declared, exported by
both libraries, bound, declared in the Rust shim; the two structs' sizes and offsets as gcc lays them out against the ctypes mirror; no
stream-taking function; the defaults; the refusals that need no device, each leaving its outputs untouched; the kernels of
vk_upsample.hip in a resource record of their own — exactly the new ones, without scratch, AGPRs, spills or a dynamic stack, the tiled
form with the LDS of its 36 x 12 footprint — and in none of the other nine."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_upsample_default_params", "vk_upsample_create", "vk_upsample_load", "vk_upsample_load_device", "vk_upsample_apply",
             "vk_upsample_apply_device", "vk_upsample_reset", "vk_upsample_get_info", "vk_upsample_destroy"]
HOOKS = ["vk_debug_upsample_set_form", "vk_debug_upsample_last_ms"]
STRUCTS = {"vk_upsample_params": ffi.UpsampleParams, "vk_upsample_info": ffi.UpsampleInfo}
SIZES = {"vk_upsample_params": 20, "vk_upsample_info": 80}
# name -> LDS bytes: the tiled form stages 36 x 12 records of three 16-byte planes
KERNELS = {
    "_Z23upsample_prepare_kernel19UpsamplePrepareArgs": 0,
    "_Z21upsample_plain_kernel12UpsampleArgs": 0,
    "_Z21upsample_tiled_kernel12UpsampleArgs": 36 * 12 * 3 * 16,
}


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
    assert lib.vk_upsample_create.argtypes == [C.c_void_p] + [C.c_uint32] * 4 + [C.POINTER(C.c_void_p)]
    assert lib.vk_upsample_load.argtypes == lib.vk_upsample_load_device.argtypes == [C.c_void_p] * 6
    assert lib.vk_upsample_apply.argtypes == lib.vk_upsample_apply_device.argtypes == [C.c_void_p, C.POINTER(ffi.UpsampleParams)] + [C.c_void_p] * 5
    assert lib.vk_upsample_get_info.argtypes == [C.c_void_p, C.POINTER(ffi.UpsampleInfo)]
    assert lib.vk_upsample_destroy.restype is None and lib.vk_upsample_destroy.argtypes == [C.c_void_p]
    assert lib.vk_debug_upsample_last_ms.argtypes == [C.c_void_p, C.POINTER(C.c_double)]
    assert all(getattr(lib, fn).restype is C.c_int for fn in FUNCTIONS[:-1] + HOOKS)
    assert re.search(r"enum \{ VK_UPSAMPLE_FORM_AUTO = 0, VK_UPSAMPLE_FORM_PLAIN = 1, VK_UPSAMPLE_FORM_TILED = 2 \};", code(header("vecchio_amd_debug.h")))
    assert (ffi.VK_UPSAMPLE_FORM_AUTO, ffi.VK_UPSAMPLE_FORM_PLAIN, ffi.VK_UPSAMPLE_FORM_TILED) == (0, 1, 2)
    assert re.search(r"enum \{ VK_UPSAMPLE_HAS_STDERR = 1, VK_UPSAMPLE_HAS_ALBEDO = 2, VK_UPSAMPLE_HAS_NORMAL = 4, VK_UPSAMPLE_HAS_DEPTH = 8 \};", code(hdr))
    assert (ffi.VK_UPSAMPLE_HAS_STDERR, ffi.VK_UPSAMPLE_HAS_ALBEDO, ffi.VK_UPSAMPLE_HAS_NORMAL, ffi.VK_UPSAMPLE_HAS_DEPTH) == (1, 2, 4, 8)
    # the names carry `upsample` and none of the words other features' ABI tests look for
    for fn in FUNCTIONS + HOOKS:
        assert "upsample" in fn and not re.search(r"denoise|tone|nlm|lpe|robust|matte|splat|adapt|temporal|glare", fn), fn
    # what the stage is not is stated where it is declared
    for words in (r"Scale 1 is not the identity", r"marginal\s+\*?\s*error", r"vk_render_guides' buffers for both\s+\*?\s*sizes"):
        assert re.search(words, hdr), words
    p = ffi.UpsampleParams(9, 9, 9, 9, 9)
    assert lib.vk_upsample_default_params(C.byref(p)) == ffi.VK_OK
    f32 = np.float32
    assert (p.sigma_z, p.normal_squarings, f32(p.albedo_floor), p.flags, p._pad) == (1.0, 7, f32(1e-3), 0, 0)


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    lo = r"color_lo: \*const f32, stderr3_lo: \*const f32, albedo_lo: \*const f32, normal_lo: \*const f32, depth_lo: \*const f32"
    hi = r"albedo_hi: \*const f32, normal_hi: \*const f32, depth_hi: \*const f32, rgb_out: \*mut f32, stderr3_out: \*mut f32"
    want = {
        "vk_upsample_default_params": r"out: \*mut vk_upsample_params\) -> c_int;",
        "vk_upsample_create": r"scene: \*mut vk_scene, w: u32, h: u32, width_hi: u32, height_hi: u32, out: \*mut \*mut vk_upsample\) -> c_int;",
        "vk_upsample_load": r"u: \*mut vk_upsample, " + lo + r"\) -> c_int;",
        "vk_upsample_load_device": r"u: \*mut vk_upsample, " + re.sub(r"(\w+_lo): \\\*const f32", r"d_\1: \\*const c_void", lo) + r"\) -> c_int;",
        "vk_upsample_apply": r"u: \*mut vk_upsample, p: \*const vk_upsample_params, " + hi + r"\) -> c_int;",
        "vk_upsample_apply_device": r"u: \*mut vk_upsample, p: \*const vk_upsample_params, d_albedo_hi: \*const c_void, d_normal_hi: \*const c_void, "
                                    r"d_depth_hi: \*const c_void, d_rgb_out: \*mut c_void, d_stderr3_out: \*mut c_void\) -> c_int;",
        "vk_upsample_reset": r"u: \*mut vk_upsample\) -> c_int;",
        "vk_upsample_get_info": r"u: \*mut vk_upsample, out: \*mut vk_upsample_info\) -> c_int;",
        "vk_upsample_destroy": r"u: \*mut vk_upsample\);",
    }
    assert sorted(want) == sorted(FUNCTIONS)
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    assert re.search(r"#\[repr\(C\)\] pub struct vk_upsample \{ _private: \[u8; 0\] \}", rs)
    import test_rust_shim_layout as R
    c, r = R.c_structs(), R.rust_structs()
    for name in STRUCTS:
        assert name in c and r.get(name) == c[name], name


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """the two structs' sizes, and every field's offset and size: the header through gcc against ctypes"""
    lines = []
    for cname, S in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in S._fields_:
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
    n = 0
    for cname, S in STRUCTS.items():
        assert seen[cname] == (SIZES[cname],) and C.sizeof(S) == SIZES[cname], cname
        for f, _ in S._fields_:
            d = getattr(S, f)
            assert seen[f"{cname}.{f}"] == (d.offset, d.size), (cname, f)
            n += 1
    assert n == 5 + 14
    assert [f for f, _ in ffi.UpsampleParams._fields_] == ["sigma_z", "normal_squarings", "albedo_floor", "flags", "_pad"]


def test_no_upsample_function_takes_a_stream():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*upsample\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args, fn
    assert seen == FUNCTIONS + HOOKS


def params(**kw):
    p = ffi.UpsampleParams(1.0, 7, 1e-3, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


NAN, INF = float("nan"), float("inf")
REFUSALS = [(dict(sigma_z=0.0), b"sigma_z must be finite and > 0"), (dict(sigma_z=-1.0), b"sigma_z must be finite and > 0"),
            (dict(sigma_z=NAN), b"sigma_z must be finite and > 0"), (dict(sigma_z=INF), b"sigma_z must be finite and > 0"),
            (dict(normal_squarings=11), b"normal_squarings must be in 0..10"), (dict(normal_squarings=0xFFFFFFFF), b"normal_squarings must be in 0..10"),
            (dict(albedo_floor=0.0), b"albedo_floor must be finite and > 0"), (dict(albedo_floor=-1e-3), b"albedo_floor must be finite and > 0"),
            (dict(albedo_floor=NAN), b"albedo_floor must be finite and > 0"), (dict(albedo_floor=INF), b"albedo_floor must be finite and > 0"),
            (dict(flags=1), b"unknown upsample flags"), (dict(_pad=1), b"unknown upsample flags")]


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    h = C.c_void_p(0x1000)                # never read: each of these is refused first
    out = C.c_void_p(0x77)
    assert lib.vk_upsample_default_params(None) == ffi.VK_ERR_BAD_ARG
    for args in ((None, 4, 4, 8, 8, C.byref(out)), (h, 4, 4, 8, 8, None)):
        assert lib.vk_upsample_create(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    for dims, word in (((1, 4, 8, 8), b"must be >= 2"), ((4, 1, 8, 8), b"must be >= 2"), ((0, 0, 8, 8), b"must be >= 2"),
                       ((9, 4, 8, 8), b"must not exceed the high size"), ((4, 9, 8, 8), b"must not exceed the high size"),
                       ((4, 4, 65536, 8), b"image too large"), ((4, 4, 8, 65536), b"image too large"), ((4, 4, 65535, 65535), b"image too large"),
                       ((4, 4, 0xFFFFFFFF, 0xFFFFFFFF), b"image too large")):
        assert lib.vk_upsample_create(h, *dims, C.byref(out)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), dims
    assert out.value == 0x77
    src, dst, se = np.full(48, 7, np.float32), np.full(192, 7, np.float32), np.full(192, 7, np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for load in (lib.vk_upsample_load, lib.vk_upsample_load_device):
        assert load(None, p(src), None, None, None, None) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
        assert load(h, None, p(src), p(src), p(src), p(src)) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    ok = params()
    for apply in (lib.vk_upsample_apply, lib.vk_upsample_apply_device):
        for args in ((None, C.byref(ok), None, None, None, p(dst), p(se)), (h, None, None, None, None, p(dst), p(se)),
                     (h, C.byref(ok), None, None, None, None, p(se))):
            assert apply(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
        for kw, word in REFUSALS:
            bad = params(**kw)
            assert apply(h, C.byref(bad), None, None, None, p(dst), p(se)) == ffi.VK_ERR_BAD_ARG, kw
            assert word in lib.vk_last_error(), (kw, lib.vk_last_error())
    assert (src == 7).all() and (dst == 7).all() and (se == 7).all()
    canary = ffi.UpsampleInfo(*([9] * 10), 9.0, 9, 9, 9)
    info = ffi.UpsampleInfo.from_buffer_copy(canary)
    assert lib.vk_upsample_get_info(None, C.byref(info)) == ffi.VK_ERR_BAD_ARG and lib.vk_upsample_get_info(h, None) == ffi.VK_ERR_BAD_ARG
    assert bytes(info) == bytes(canary)
    assert lib.vk_upsample_reset(None) == ffi.VK_ERR_BAD_ARG
    lib.vk_upsample_destroy(None)         # nothing
    assert lib.vk_debug_upsample_set_form(None, 0) == ffi.VK_ERR_BAD_ARG
    ms = C.c_double(7)
    assert lib.vk_debug_upsample_last_ms(None, C.byref(ms)) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_upsample_last_ms(h, None) == ffi.VK_ERR_BAD_ARG
    assert ms.value == 7


def resources(path):
    out = {}
    for blk in open(path).read().split("Name: ")[1:]:
        name = blk.split("\n")[0].strip()
        assert name not in out
        get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
        out[name] = dict(vgprs=get("VGPRs"), agprs=get("AGPRs"), scratch=get("ScratchSize [bytes/lane]"), scratch_ops=get("ScratchOps"),
                         spills=get("VGPRs Spill"), sgpr_spills=get("SGPRs Spill"), occupancy=get("Occupancy [waves/SIMD]"),
                         lds=get("LDS Size [bytes/block]"), dynamic_stack="Dynamic Stack: True" in blk)
    return out


def test_the_kernels_are_new_and_in_a_record_of_their_own(built):
    """kernel_resources_upsample.txt lists exactly the kernels of vk_upsample.hip, each once — the prepare pass, the plain and the tiled
    filter —: no scratch, no scratch instructions, no AGPRs, no spills, no dynamic stack, at least 7 waves per SIMD; the tiled form's LDS
    is its 36 x 12 footprint; the other nine records and vk_kernels.h hold none of them"""
    mine = resources(build.kernel_resources_upsample_path())
    assert sorted(mine) == sorted(KERNELS), sorted(mine)
    for name, r in mine.items():
        assert r["agprs"] == 0 and r["scratch"] == 0 and r["scratch_ops"] == 0 and r["spills"] == 0 and r["sgpr_spills"] == 0, (name, r)
        assert not r["dynamic_stack"], name
        assert r["lds"] == KERNELS[name] and r["vgprs"] <= 72 and r["occupancy"] >= 7, (name, r)
    for path in (build.kernel_resources_path(), build.kernel_resources_adapt_path(), build.kernel_resources_splat_path(),
                 build.kernel_resources_matte_path(), build.kernel_resources_robust_path(), build.kernel_resources_lpe_path(),
                 build.kernel_resources_tone_path(), build.kernel_resources_nlm_path(), build.kernel_resources_glare_path()):
        assert "upsample" not in open(path).read().lower(), path
    src = open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_upsample.hip")).read()
    assert len(re.findall(r"__global__", src)) == 3 and "asm" not in src
    assert "asm" not in open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_upsample.h")).read()
    assert "upsample" not in open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_kernels.h")).read().lower()
