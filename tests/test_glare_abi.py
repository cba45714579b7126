"""Glare (vk_glare_*, additive symbols of ABI 7) on the CPU: the six functions and the two debug hooks declared, exported by both
libraries, bound, declared in the Rust shim; the two structs' sizes and offsets as gcc lays them out against the ctypes mirror; no
stream-taking function; the defaults; the refusals that need no device, each leaving its outputs untouched; the kernels of vk_glare.hip
in a resource record of their own — exactly the new ones, without scratch, AGPRs, spills or a dynamic stack, with the LDS each was built
with — and in none of the other eight."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_glare_default_params", "vk_glare_create", "vk_glare_apply", "vk_glare_apply_device", "vk_glare_get_info", "vk_glare_destroy"]
HOOKS = ["vk_debug_glare_set_form", "vk_debug_glare_last_ms"]
STRUCTS = {"vk_glare_params": ffi.GlareParams, "vk_glare_info": ffi.GlareInfo}
SIZES = {"vk_glare_params": 24, "vk_glare_info": 48}
# name -> (LDS bytes, VGPRs, waves per SIMD) as the build gives them (DESIGN.md "Glare").  The LDS down kernel: a 66 x 18 source tile and
# its 32 x 18 x pass, three components.  The two-level kernel: 70 x 38 of the frame, its 34 x 38 x pass, level 1's 34 x 18 tile and its
# 16 x 18 x pass.  The tail: 8192 + 6144 + 1792 floats of one component.
KERNELS = {
    "_Z17glare_down_kernelILb1ELb0EEv13GlareDownArgs": (0, 62, 8),
    "_Z17glare_down_kernelILb0ELb0EEv13GlareDownArgs": (0, 72, 7),
    "_Z17glare_down_kernelILb1ELb1EEv13GlareDownArgs": (12 * (66 * 18 + 32 * 18), 17, 7),
    "_Z17glare_down_kernelILb0ELb1EEv13GlareDownArgs": (12 * (66 * 18 + 32 * 18), 10, 7),
    "_Z18glare_down2_kernel14GlareDown2Args": (12 * (70 * 38 + 34 * 38 + 34 * 18 + 16 * 18), 36, 2),
    "_Z15glare_up_kernel11GlareUpArgs": (0, 28, 8),
    "_Z22glare_composite_kernel18GlareCompositeArgs": (0, 28, 8),
    "_Z17glare_tail_kernel13GlareTailArgs": (4 * (8192 + 6144 + 1792), 70, 7),
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
    assert lib.vk_glare_create.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    assert lib.vk_glare_apply.argtypes == lib.vk_glare_apply_device.argtypes == [C.c_void_p, C.POINTER(ffi.GlareParams), C.c_void_p, C.c_void_p]
    assert lib.vk_glare_get_info.argtypes == [C.c_void_p, C.POINTER(ffi.GlareInfo)]
    assert lib.vk_glare_destroy.restype is None and lib.vk_glare_destroy.argtypes == [C.c_void_p]
    assert lib.vk_debug_glare_last_ms.argtypes == [C.c_void_p, C.POINTER(C.c_double)]
    assert all(getattr(lib, fn).restype is C.c_int for fn in FUNCTIONS[:-1] + HOOKS)
    assert re.search(r"enum \{ VK_GLARE_FORM_AUTO = 0, VK_GLARE_FORM_PLAIN = 1, VK_GLARE_FORM_FUSED = 2 \};", code(header("vecchio_amd_debug.h")))
    assert (ffi.VK_GLARE_FORM_AUTO, ffi.VK_GLARE_FORM_PLAIN, ffi.VK_GLARE_FORM_FUSED) == (0, 1, 2)
    # the names carry `glare` and none of the words other features' ABI tests look for
    for fn in FUNCTIONS + HOOKS:
        assert "glare" in fn and not re.search(r"denoise|tone|nlm|lpe|robust|matte|splat|adapt|temporal", fn), fn
    # tone's contract points here
    assert re.search(r"No bloom or glare.*?vk_glare_\*", hdr, flags=re.S)
    p = ffi.GlareParams(9, 9, 9, 9, 9, 9)
    assert lib.vk_glare_default_params(C.byref(p)) == ffi.VK_OK
    f32 = np.float32
    assert (p.levels, f32(p.strength), p.falloff, p.threshold, p.flags, p._pad) == (6, f32(0.15), 1.0, 0.0, 0, 0)


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    want = {
        "vk_glare_default_params": r"out: \*mut vk_glare_params\) -> c_int;",
        "vk_glare_create": r"scene: \*mut vk_scene, width: u32, height: u32, out: \*mut \*mut vk_glare\) -> c_int;",
        "vk_glare_apply": r"g: \*mut vk_glare, p: \*const vk_glare_params, rgb_in: \*const f32, rgb_out: \*mut f32\) -> c_int;",
        "vk_glare_apply_device": r"g: \*mut vk_glare, p: \*const vk_glare_params, d_rgb_in: \*const c_void, d_rgb_out: \*mut c_void\) -> c_int;",
        "vk_glare_get_info": r"g: \*mut vk_glare, out: \*mut vk_glare_info\) -> c_int;",
        "vk_glare_destroy": r"g: \*mut vk_glare\);",
    }
    assert sorted(want) == sorted(FUNCTIONS)
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    assert re.search(r"#\[repr\(C\)\] pub struct vk_glare \{ _private: \[u8; 0\] \}", rs)
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
    assert n == 6 + 9
    assert [f for f, _ in ffi.GlareParams._fields_] == ["levels", "strength", "falloff", "threshold", "flags", "_pad"]


def test_no_glare_function_takes_a_stream():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*glare\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args, fn
    assert seen == FUNCTIONS + HOOKS


def params(**kw):
    p = ffi.GlareParams(6, 0.15, 1.0, 0.0, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


NAN, INF = float("nan"), float("inf")
REFUSALS = [(dict(levels=0), b"levels must be in 1..8"), (dict(levels=9), b"levels must be in 1..8"), (dict(levels=0xFFFFFFFF), b"levels must be in 1..8"),
            (dict(strength=-0.01), b"strength must be in [0, 1]"), (dict(strength=1.01), b"strength must be in [0, 1]"),
            (dict(strength=NAN), b"strength must be in [0, 1]"), (dict(strength=INF), b"strength must be in [0, 1]"),
            (dict(falloff=0.0), b"falloff must be finite and > 0"), (dict(falloff=-1.0), b"falloff must be finite and > 0"),
            (dict(falloff=NAN), b"falloff must be finite and > 0"), (dict(falloff=INF), b"falloff must be finite and > 0"),
            (dict(threshold=-0.5), b"threshold must be finite and >= 0"), (dict(threshold=NAN), b"threshold must be finite and >= 0"),
            (dict(threshold=INF), b"threshold must be finite and >= 0"), (dict(flags=1), b"unknown glare flags"), (dict(_pad=1), b"unknown glare flags")]


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    h = C.c_void_p(0x1000)                # never read: each of these is refused first
    out = C.c_void_p(0x77)
    assert lib.vk_glare_default_params(None) == ffi.VK_ERR_BAD_ARG
    for args in ((None, 4, 4, C.byref(out)), (h, 4, 4, None)):
        assert lib.vk_glare_create(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    for dims, word in (((0, 4), b"width and height must be >= 1"), ((4, 0), b"width and height must be >= 1"), ((65536, 1), b"image too large"),
                       ((1, 65536), b"image too large"), ((65535, 65535), b"image too large"), ((0xFFFFFFFF, 0xFFFFFFFF), b"image too large")):
        assert lib.vk_glare_create(h, *dims, C.byref(out)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), dims
    assert out.value == 0x77
    src, dst = np.full(48, 7, np.float32), np.full(48, 7, np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    ok = params()
    for apply in (lib.vk_glare_apply, lib.vk_glare_apply_device):
        for args in ((None, C.byref(ok), p(src), p(dst)), (h, None, p(src), p(dst)), (h, C.byref(ok), None, p(dst)), (h, C.byref(ok), p(src), None)):
            assert apply(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
        for kw, word in REFUSALS:
            bad = params(**kw)
            assert apply(h, C.byref(bad), p(src), p(dst)) == ffi.VK_ERR_BAD_ARG, kw
            assert word in lib.vk_last_error(), (kw, lib.vk_last_error())
    assert (src == 7).all() and (dst == 7).all()
    canary = ffi.GlareInfo(9, 9, 9, 9, 9, 9, 9, 9.0, 9)
    info = ffi.GlareInfo.from_buffer_copy(canary)
    assert lib.vk_glare_get_info(None, C.byref(info)) == ffi.VK_ERR_BAD_ARG and lib.vk_glare_get_info(h, None) == ffi.VK_ERR_BAD_ARG
    assert bytes(info) == bytes(canary)
    lib.vk_glare_destroy(None)            # nothing
    assert lib.vk_debug_glare_set_form(None, 0) == ffi.VK_ERR_BAD_ARG
    ms = C.c_double(7)
    assert lib.vk_debug_glare_last_ms(None, C.byref(ms)) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_glare_last_ms(h, None) == ffi.VK_ERR_BAD_ARG
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
    """kernel_resources_glare.txt lists exactly the kernels of vk_glare.hip, each once — the down pass in its plain and LDS forms from the
    frame and from a plane, the two-level down pass, the up pass, the composite and the tail —: no scratch, no scratch instructions, no
    AGPRs, no spills, no dynamic stack; at most 64 KB of LDS; VGPRs and occupancy as the build gives them; the other eight records and
    vk_kernels.h hold none of them"""
    mine = resources(build.kernel_resources_glare_path())
    assert sorted(mine) == sorted(KERNELS), sorted(mine)
    for name, r in mine.items():
        assert r["agprs"] == 0 and r["scratch"] == 0 and r["scratch_ops"] == 0 and r["spills"] == 0 and r["sgpr_spills"] == 0, (name, r)
        assert not r["dynamic_stack"], name
        assert (r["lds"], r["vgprs"], r["occupancy"]) == KERNELS[name] and r["lds"] <= 65536, (name, r)
    for path in (build.kernel_resources_path(), build.kernel_resources_adapt_path(), build.kernel_resources_splat_path(),
                 build.kernel_resources_matte_path(), build.kernel_resources_robust_path(), build.kernel_resources_lpe_path(),
                 build.kernel_resources_tone_path(), build.kernel_resources_nlm_path()):
        assert "glare" not in open(path).read().lower(), path
    src = open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_glare.hip")).read()
    assert len(re.findall(r"__global__", src)) == 5 and "asm" not in src
    assert "asm" not in open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_glare.h")).read()
    assert "glare" not in open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_kernels.h")).read().lower()
