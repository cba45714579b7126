"""Non-local means (vk_nlm_*, additive symbols of ABI 7) on the CPU: the nine functions and the two debug hooks declared, exported by both
libraries, bound, declared in the Rust shim; the two structs' sizes and offsets as gcc lays them out against the ctypes mirror; no
stream-taking function; the defaults; the refusals that need no device, each leaving its outputs untouched; the kernels of vk_nlm.hip
in a resource record of their own — exactly the new ones, without scratch, AGPRs, spills or a dynamic stack, with the LDS each form was
built with — and in none of the other seven."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_nlm_default_params", "vk_nlm_create", "vk_nlm_load", "vk_nlm_load_device", "vk_nlm_filter", "vk_nlm_filter_device",
             "vk_nlm_reset", "vk_nlm_get_info", "vk_nlm_destroy"]
HOOKS = ["vk_debug_nlm_set_form", "vk_debug_nlm_last_ms"]
STRUCTS = {"vk_nlm_params": ffi.NlmParams, "vk_nlm_info": ffi.NlmInfo}
SIZES = {"vk_nlm_params": 24, "vk_nlm_info": 56}
# name -> (LDS bytes, VGPRs, waves per SIMD) as the build gives them (DESIGN.md "Non-local means").  The tiled form's LDS: six staged
# planes of (32 + 2 halo) x (8 + 2 halo) floats, the pair plane and its count (38 x 14 each), the row sums and their count (32 x 14 each).
KERNELS = {
    "_Z18nlm_prepare_kernel14NlmPrepareArgs": (0, 35, 8),
    "_Z17nlm_filter_kernelILj1ELi0EEv13NlmFilterArgs": (0, 61, 8),
    "_Z17nlm_filter_kernelILj2ELi6EEv13NlmFilterArgs": (24 * 44 * 20 + 8 * 38 * 14 + 8 * 32 * 14, 37, 5),
    "_Z17nlm_filter_kernelILj2ELi13EEv13NlmFilterArgs": (24 * 58 * 34 + 8 * 38 * 14 + 8 * 32 * 14, 37, 2),
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
    assert lib.vk_nlm_create.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    assert lib.vk_nlm_load.argtypes == lib.vk_nlm_load_device.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.vk_nlm_filter.argtypes == lib.vk_nlm_filter_device.argtypes == [C.c_void_p, C.POINTER(ffi.NlmParams), C.c_void_p, C.c_void_p]
    assert lib.vk_nlm_get_info.argtypes == [C.c_void_p, C.POINTER(ffi.NlmInfo)]
    assert lib.vk_nlm_destroy.restype is None and lib.vk_nlm_destroy.argtypes == [C.c_void_p]
    assert lib.vk_debug_nlm_last_ms.argtypes == [C.c_void_p, C.POINTER(C.c_double * 2)]
    assert all(getattr(lib, fn).restype is C.c_int for fn in FUNCTIONS[:-1] + HOOKS)
    assert re.search(r"enum \{ VK_NLM_FORM_AUTO = 0, VK_NLM_FORM_PLAIN = 1, VK_NLM_FORM_TILED = 2 \};", code(header("vecchio_amd_debug.h")))
    assert (ffi.VK_NLM_FORM_AUTO, ffi.VK_NLM_FORM_PLAIN, ffi.VK_NLM_FORM_TILED) == (0, 1, 2)
    # the names carry `nlm` and none of the words other features' ABI tests look for
    for fn in FUNCTIONS + HOOKS:
        assert "nlm" in fn and not re.search(r"denoise|tone|lpe|robust|matte|splat|adapt|temporal", fn), fn
    p = ffi.NlmParams(9, 9, 9, 9, 9, 9)
    assert lib.vk_nlm_default_params(C.byref(p)) == ffi.VK_OK
    f32 = np.float32
    assert (p.search_radius, p.patch_radius, f32(p.k), p.alpha, f32(p.albedo_floor), p.flags) == (7, 3, f32(0.45), 1.0, f32(1e-3), 0)


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    want = {
        "vk_nlm_default_params": r"out: \*mut vk_nlm_params\) -> c_int;",
        "vk_nlm_create": r"scene: \*mut vk_scene, width: u32, height: u32, out: \*mut \*mut vk_nlm\) -> c_int;",
        "vk_nlm_load": r"h: \*mut vk_nlm, color: \*const f32, stderr3: \*const f32, albedo: \*const f32\) -> c_int;",
        "vk_nlm_load_device": r"h: \*mut vk_nlm, d_color: \*const c_void, d_stderr3: \*const c_void, d_albedo: \*const c_void\) -> c_int;",
        "vk_nlm_filter": r"h: \*mut vk_nlm, p: \*const vk_nlm_params, rgb_out: \*mut f32, stderr3_out: \*mut f32\) -> c_int;",
        "vk_nlm_filter_device": r"h: \*mut vk_nlm, p: \*const vk_nlm_params, d_rgb_out: \*mut c_void, d_stderr3_out: \*mut c_void\) -> c_int;",
        "vk_nlm_reset": r"h: \*mut vk_nlm\) -> c_int;",
        "vk_nlm_get_info": r"h: \*mut vk_nlm, out: \*mut vk_nlm_info\) -> c_int;",
        "vk_nlm_destroy": r"h: \*mut vk_nlm\);",
    }
    assert sorted(want) == sorted(FUNCTIONS)
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    assert re.search(r"#\[repr\(C\)\] pub struct vk_nlm \{ _private: \[u8; 0\] \}", rs)
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
    assert n == 6 + 10
    assert [f for f, _ in ffi.NlmParams._fields_] == ["search_radius", "patch_radius", "k", "alpha", "albedo_floor", "flags"]


def test_no_nlm_function_takes_a_stream():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*nlm\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args, fn
    assert seen == FUNCTIONS + HOOKS


def params(**kw):
    p = ffi.NlmParams(7, 3, 0.45, 1.0, 1e-3, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


REFUSALS = [(dict(search_radius=0), b"search_radius must be in 1..10"), (dict(search_radius=11), b"search_radius must be in 1..10"),
            (dict(search_radius=0xFFFFFFFF), b"search_radius must be in 1..10"), (dict(patch_radius=4), b"patch_radius must be in 0..3"),
            (dict(k=0.0), b"k must be finite and > 0"), (dict(k=-0.5), b"k must be finite and > 0"), (dict(k=float("nan")), b"k must be finite and > 0"),
            (dict(k=float("inf")), b"k must be finite and > 0"), (dict(alpha=-0.1), b"alpha must be finite and >= 0"),
            (dict(alpha=float("nan")), b"alpha must be finite and >= 0"), (dict(alpha=float("inf")), b"alpha must be finite and >= 0"),
            (dict(albedo_floor=0.0), b"albedo_floor must be finite and > 0"), (dict(albedo_floor=-1.0), b"albedo_floor must be finite and > 0"),
            (dict(albedo_floor=float("nan")), b"albedo_floor must be finite and > 0"),
            (dict(albedo_floor=float("inf")), b"albedo_floor must be finite and > 0"), (dict(flags=1), b"unknown nlm flags")]


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    h = C.c_void_p(0x1000)                # never read: each of these is refused first
    out = C.c_void_p(0x77)
    assert lib.vk_nlm_default_params(None) == ffi.VK_ERR_BAD_ARG
    for args in ((None, 4, 4, C.byref(out)), (h, 4, 4, None)):
        assert lib.vk_nlm_create(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    for dims, word in (((0, 4), b"width and height must be >= 1"), ((4, 0), b"width and height must be >= 1"), ((65536, 1), b"image too large"),
                       ((1, 65536), b"image too large"), ((65535, 65535), b"image too large"), ((0xFFFFFFFF, 0xFFFFFFFF), b"image too large")):
        assert lib.vk_nlm_create(h, *dims, C.byref(out)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), dims
    assert out.value == 0x77
    img = np.full(48, 7, np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for load in (lib.vk_nlm_load, lib.vk_nlm_load_device):
        for args in ((None, p(img), p(img), p(img)), (h, None, p(img), p(img)), (h, p(img), None, p(img))):
            assert load(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    rgb, se = np.full(48, 7, np.float32), np.full(48, 7, np.float32)
    ok = params()
    for flt in (lib.vk_nlm_filter, lib.vk_nlm_filter_device):
        for args in ((None, C.byref(ok), p(rgb), p(se)), (h, None, p(rgb), p(se)), (h, C.byref(ok), None, p(se))):
            assert flt(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
        for kw, word in REFUSALS:
            bad = params(**kw)
            assert flt(h, C.byref(bad), p(rgb), p(se)) == ffi.VK_ERR_BAD_ARG, kw
            assert word in lib.vk_last_error(), (kw, lib.vk_last_error())
    assert (rgb == 7).all() and (se == 7).all() and (img == 7).all()
    assert lib.vk_nlm_reset(None) == ffi.VK_ERR_BAD_ARG and b"null nlm handle" in lib.vk_last_error()
    canary = ffi.NlmInfo(9, 9, 9, 9, 9, 9, 9, 9, 9.0, 9)
    info = ffi.NlmInfo.from_buffer_copy(canary)
    assert lib.vk_nlm_get_info(None, C.byref(info)) == ffi.VK_ERR_BAD_ARG and lib.vk_nlm_get_info(h, None) == ffi.VK_ERR_BAD_ARG
    assert bytes(info) == bytes(canary)
    lib.vk_nlm_destroy(None)              # nothing
    assert lib.vk_debug_nlm_set_form(None, 0) == ffi.VK_ERR_BAD_ARG
    ms = (C.c_double * 2)(7, 7)
    assert lib.vk_debug_nlm_last_ms(None, C.byref(ms)) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_nlm_last_ms(h, None) == ffi.VK_ERR_BAD_ARG
    assert list(ms) == [7, 7]


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
    """kernel_resources_nlm.txt lists exactly the kernels of vk_nlm.hip, each once — prepare, the plain form and the tiled form's two
    instances (a halo of up to 6 and of up to 13 pixels) —: no scratch, no scratch instructions, no AGPRs, no spills, no dynamic stack; the
    tiled instances hold their planes in at most 64 KB of LDS, the others nothing; VGPRs and occupancy as the build gives them; the
    other seven records and vk_kernels.h hold none of them"""
    mine = resources(build.kernel_resources_nlm_path())
    assert sorted(mine) == sorted(KERNELS), sorted(mine)
    for name, r in mine.items():
        assert r["agprs"] == 0 and r["scratch"] == 0 and r["scratch_ops"] == 0 and r["spills"] == 0 and r["sgpr_spills"] == 0, (name, r)
        assert not r["dynamic_stack"], name
        assert (r["lds"], r["vgprs"], r["occupancy"]) == KERNELS[name] and r["lds"] <= 65536, (name, r)
    for path in (build.kernel_resources_path(), build.kernel_resources_adapt_path(), build.kernel_resources_splat_path(),
                 build.kernel_resources_matte_path(), build.kernel_resources_robust_path(), build.kernel_resources_lpe_path(),
                 build.kernel_resources_tone_path()):
        assert "nlm" not in open(path).read().lower(), path
    src = open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_nlm.hip")).read()
    assert len(re.findall(r"__global__", src)) == 2 and "asm" not in src
    assert "asm" not in open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_nlm.h")).read()
    assert "nlm" not in open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_kernels.h")).read().lower()
