"""Light-path layers (vk_lpe_*, additive symbols of ABI 7) on the CPU: the eight functions and the three debug hooks declared, exported
by both libraries, bound, declared in the Rust shim; the three structs' sizes and offsets as gcc lays them out against the ctypes mirror;
no stream-taking function; the refusals that need no device, each leaving its outputs untouched; the kernels of vk_lpe.hip in a resource
record of their own — exactly the three new ones, without scratch, AGPRs or a dynamic stack and within 32 VGPRs — and in none of the
other five."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_lpe_create", "vk_lpe_step", "vk_lpe_tags", "vk_lpe_deposit", "vk_lpe_resolve", "vk_lpe_reset", "vk_lpe_get_info",
             "vk_lpe_destroy"]
HOOKS = ["vk_debug_lpe_sums", "vk_debug_lpe_set_tags", "vk_debug_lpe_last_ms"]
STRUCTS = {"vk_lpe_rule": ffi.LpeRule, "vk_lpe_params": ffi.LpeParams, "vk_lpe_info": ffi.LpeInfo}
KERNELS = ["_Z17lpe_record_kernel13LpeRecordArgs", "_Z18lpe_deposit_kernel14LpeDepositArgs", "_Z18lpe_resolve_kernel14LpeResolveArgs"]


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
    assert lib.vk_lpe_create.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(ffi.LpeParams), C.POINTER(C.c_void_p)]
    assert lib.vk_lpe_step.argtypes == [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ffi.PathsStepInfo)]
    assert lib.vk_lpe_tags.argtypes == [C.c_void_p] * 4 and lib.vk_lpe_deposit.argtypes == [C.c_void_p, C.c_void_p]
    assert lib.vk_lpe_resolve.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    assert lib.vk_lpe_reset.argtypes == [C.c_void_p] and lib.vk_lpe_get_info.argtypes == [C.c_void_p, C.POINTER(ffi.LpeInfo)]
    assert lib.vk_lpe_destroy.restype is None and lib.vk_lpe_destroy.argtypes == [C.c_void_p]
    assert lib.vk_debug_lpe_sums.argtypes == [C.c_void_p, C.c_void_p] and lib.vk_debug_lpe_set_tags.argtypes == [C.c_void_p] * 4
    assert lib.vk_debug_lpe_last_ms.argtypes == [C.c_void_p, C.POINTER(C.c_double * 3)]
    assert all(getattr(lib, fn).restype is C.c_int for fn in FUNCTIONS[:-1] + HOOKS)
    assert (ffi.VK_LPE_SKY, ffi.VK_LPE_EMIT, ffi.VK_LPE_OTHER, ffi.VK_LPE_BAD, ffi.VK_LPE_ALL) == (1, 5, 14, 15, 0xFFFFFFFF)
    assert re.search(r"enum \{ VK_LPE_SKY = 1, VK_LPE_EMIT = 5, VK_LPE_OTHER = 14, VK_LPE_BAD = 15 \};", code(hdr))
    assert re.search(r"#define VK_LPE_ALL 0xFFFFFFFFu\b", hdr)
    assert ffi.VK_LPE_EMIT == 2 + ffi.VK_MAT_DIFFUSE_LIGHT


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    want = {
        "vk_lpe_create": r"scene: \*mut vk_scene, width: u32, height: u32, samples_per_pixel: u32, capacity: u64, lp: \*const vk_lpe_params, "
                         r"out: \*mut \*mut vk_lpe\) -> c_int;",
        "vk_lpe_step": r"s: \*mut vk_lpe, batch: \*mut vk_paths, max_bounces: u32, info: \*mut vk_paths_step_info\) -> c_int;",
        "vk_lpe_tags": r"s: \*mut vk_lpe, batch: \*mut vk_paths, sig: \*mut u32, term: \*mut u32\) -> c_int;",
        "vk_lpe_deposit": r"s: \*mut vk_lpe, batch: \*mut vk_paths\) -> c_int;",
        "vk_lpe_resolve": r"s: \*mut vk_lpe, layer: u32, n: u32, rgb_out: \*mut f32, share_out: \*mut f32\) -> c_int;",
        "vk_lpe_reset": r"s: \*mut vk_lpe\) -> c_int;",
        "vk_lpe_get_info": r"s: \*mut vk_lpe, out: \*mut vk_lpe_info\) -> c_int;",
        "vk_lpe_destroy": r"s: \*mut vk_lpe\);",
    }
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    assert re.search(r"#\[repr\(C\)\] pub struct vk_lpe \{ _private: \[u8; 0\] \}", rs)
    for n, v in (("VK_LPE_SKY", "1"), ("VK_LPE_EMIT", "5"), ("VK_LPE_OTHER", "14"), ("VK_LPE_BAD", "15"), ("VK_LPE_ALL", "0xFFFF_FFFF")):
        assert re.search(rf"pub const {n}: u32 = {v};", rs), n
    fields = {
        "vk_lpe_rule": "pub sig_mask: u32, pub sig_value: u32, pub status_mask: u32, pub depth_min: u32, pub depth_max: u32, pub emitter: u32, "
                       "pub layer: u32, pub _pad: u32",
        "vk_lpe_params": "pub n_layers: u32, pub rest_layer: u32, pub n_rules: u32, pub _pad: u32, pub rules: *const vk_lpe_rule",
        "vk_lpe_info": "pub width: u32, pub height: u32, pub samples_per_pixel: u32, pub n_layers: u32, pub rest_layer: u32, pub n_rules: u32, "
                       "pub capacity: u64, pub deposited: u64, pub dropped: u64, pub clamped: u64, pub skipped: u64, pub deposits: u64, "
                       "pub recorded: u64",
    }
    for name, f in fields.items():
        m = re.search(r"#\[repr\(C\)\][^{;]*?pub struct " + name + r"\s*\{(.*?)\}", rs, flags=re.S)
        assert m and " ".join(m.group(1).split()) == f, name


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """vk_lpe_rule 32 bytes, vk_lpe_params 24, vk_lpe_info 80, and every field's offset and size: the header through gcc against ctypes"""
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
    assert seen["vk_lpe_rule"] == (32,) and seen["vk_lpe_params"] == (24,) and seen["vk_lpe_info"] == (80,)
    n = 0
    for cname, T in STRUCTS.items():
        assert C.sizeof(T) == seen[cname][0]
        for f, _ in T._fields_:
            d = getattr(T, f)
            assert seen[f"{cname}.{f}"] == (d.offset, d.size), (cname, f)
            n += 1
    assert n == 8 + 5 + 13
    assert [f for f, _ in ffi.LpeRule._fields_] == ["sig_mask", "sig_value", "status_mask", "depth_min", "depth_max", "emitter", "layer", "_pad"]
    assert [f for f, _ in ffi.LpeParams._fields_] == ["n_layers", "rest_layer", "n_rules", "_pad", "rules"]
    # the step's info struct is vk_paths_step's
    assert re.search(r"int vk_lpe_step\(vk_lpe \*s, vk_paths \*batch, uint32_t max_bounces, vk_paths_step_info \*info\);", code(header()))


def test_no_lpe_function_takes_a_stream():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*lpe\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args and "void *" not in args and "_device" not in fn, fn
    assert seen == FUNCTIONS + HOOKS


def rule(**kw):
    f = dict(sig_mask=0, sig_value=0, status_mask=21, depth_min=0, depth_max=0xFFFFFFFF, emitter=0xFFFFFFFF, layer=0, _pad=0)
    f.update(kw)
    return ffi.LpeRule(*(f[k] for k, _ in ffi.LpeRule._fields_))


def params(n_layers=4, rest=0, rules=(), n_rules=None, pad=0):
    arr = (ffi.LpeRule * max(1, len(rules)))(*rules)
    lp = ffi.LpeParams(n_layers, rest, len(rules) if n_rules is None else n_rules, pad, arr if rules else None)
    lp._keep = arr
    return lp


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    h = C.c_void_p(0x1000)                # never read: each of these is refused first
    out = C.c_void_p(0x77)
    ok = params(rules=[rule(layer=3)])

    def create(lp, w=4, hh=4, spp=1, cap=16, scene=h, o=out):
        return lib.vk_lpe_create(scene, w, hh, spp, cap, C.byref(lp) if lp is not None else None, C.byref(o) if o is not None else None)

    for kw in (dict(scene=None), dict(lp=None), dict(o=None)):
        a = dict(lp=ok)
        a.update(kw)
        assert create(**a) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    for kw, word in ((dict(w=0), b"width and height must be >= 1"), (dict(hh=0), b"width and height must be >= 1"),
                     (dict(w=8192, hh=4097), b"width * height * n_layers exceeds 2^27"), (dict(w=0xFFFFFFFF, hh=0xFFFFFFFF), b"exceeds 2^27"),
                     (dict(spp=0), b"samples_per_pixel must be in 1..2^26"), (dict(spp=(1 << 26) + 1), b"samples_per_pixel must be in 1..2^26"),
                     (dict(cap=0), b"capacity must be in 1..2^24"), (dict(cap=(1 << 24) + 1), b"capacity must be in 1..2^24")):
        assert create(ok, **kw) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), kw
    for lp, word in ((params(n_layers=0), b"n_layers must be in 1..16"), (params(n_layers=17), b"n_layers must be in 1..16"),
                     (params(n_layers=4, rest=4), b"rest_layer is not below n_layers"), (params(n_rules=33), b"n_rules must be in 0..32"),
                     (params(n_rules=1), b"null rules with n_rules > 0"), (params(pad=1), b"_pad must be 0"),
                     (params(rules=[rule(), rule(sig_mask=0xF0, sig_value=0x11)]), b"sig_value has bits outside its sig_mask"),
                     (params(rules=[rule(status_mask=0)]), b"status_mask must name MISS, ENDED or CULLED"),
                     (params(rules=[rule(status_mask=2)]), b"status_mask must name MISS, ENDED or CULLED"),
                     (params(rules=[rule(status_mask=21 | 8)]), b"status_mask must name MISS, ENDED or CULLED"),
                     (params(rules=[rule(status_mask=1 << 31)]), b"status_mask must name MISS, ENDED or CULLED"),
                     (params(rules=[rule(depth_min=3, depth_max=2)]), b"depth_min exceeds its depth_max"),
                     (params(rules=[rule(layer=4)]), b"layer is not below n_layers"), (params(rules=[rule(_pad=1)]), b"a rule's _pad must be 0")):
        assert create(lp) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), word
    # 4096 x 4096 x 8 is 2^27 exactly: admitted as far as the arguments go (9 layers are not)
    assert create(params(n_layers=9), w=4096, hh=4096) == ffi.VK_ERR_BAD_ARG and b"exceeds 2^27" in lib.vk_last_error()
    assert out.value == 0x77
    info = ffi.PathsStepInfo()
    before = bytes(info)
    for a, b in ((None, h), (h, None)):
        assert lib.vk_lpe_step(a, b, 1, C.byref(info)) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
        assert lib.vk_lpe_deposit(a, b) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
        sig = np.full(4, 7, np.uint32)
        assert lib.vk_lpe_tags(a, b, sig.ctypes.data, sig.ctypes.data) == ffi.VK_ERR_BAD_ARG and (sig == 7).all()
        assert lib.vk_debug_lpe_set_tags(a, b, sig.ctypes.data, sig.ctypes.data) == ffi.VK_ERR_BAD_ARG
    assert bytes(info) == before
    img, share = np.full(12, 7, np.float32), np.full(4, 7, np.float32)
    assert lib.vk_lpe_resolve(None, 0, 1, img.ctypes.data, share.ctypes.data) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_lpe_resolve(h, 0, 1, None, share.ctypes.data) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    assert lib.vk_lpe_reset(None) == ffi.VK_ERR_BAD_ARG and b"null tracker" in lib.vk_last_error()
    li = ffi.LpeInfo(*([9] * 13))
    assert lib.vk_lpe_get_info(None, C.byref(li)) == ffi.VK_ERR_BAD_ARG and lib.vk_lpe_get_info(h, None) == ffi.VK_ERR_BAD_ARG
    assert bytes(li) == bytes(ffi.LpeInfo(*([9] * 13)))
    lib.vk_lpe_destroy(None)              # nothing
    sums = np.full(8, 7, np.int64)
    assert lib.vk_debug_lpe_sums(None, sums.ctypes.data) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_lpe_sums(h, None) == ffi.VK_ERR_BAD_ARG
    ms = (C.c_double * 3)(7, 7, 7)
    assert lib.vk_debug_lpe_last_ms(None, C.byref(ms)) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_lpe_last_ms(h, None) == ffi.VK_ERR_BAD_ARG
    assert list(ms) == [7, 7, 7] and (sums == 7).all() and (img == 7).all() and (share == 7).all()


def resources(path):
    out = {}
    for blk in open(path).read().split("Name: ")[1:]:
        name = blk.split("\n")[0].strip()
        assert name not in out
        get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
        out[name] = dict(vgprs=get("VGPRs"), agprs=get("AGPRs"), scratch=get("ScratchSize [bytes/lane]"), scratch_ops=get("ScratchOps"),
                         occupancy=get("Occupancy [waves/SIMD]"), lds=get("LDS Size [bytes/block]"), dynamic_stack="Dynamic Stack: True" in blk,
                         spills=get("VGPRs Spill") + get("SGPRs Spill"))
    return out


def test_the_kernels_are_new_and_in_a_record_of_their_own(built):
    """kernel_resources_lpe.txt lists exactly the kernels of vk_lpe.hip, each once: no scratch (the rules are read from the argument
    record, never copied), no AGPRs, no LDS, no dynamic stack, at most 32 VGPRs — the bounds tests/test_roulette_abi.py puts on its
    kernel; the other five records hold none of them"""
    mine = resources(build.kernel_resources_lpe_path())
    assert sorted(mine) == sorted(KERNELS), sorted(mine)
    for name, r in mine.items():
        assert r["agprs"] == 0 and r["scratch"] == 0 and r["scratch_ops"] == 0 and not r["dynamic_stack"] and r["lds"] == 0, (name, r)
        assert r["vgprs"] <= 32 and r["occupancy"] >= 8 and r["spills"] == 0, (name, r)
    for path in (build.kernel_resources_path(), build.kernel_resources_adapt_path(), build.kernel_resources_splat_path(),
                 build.kernel_resources_matte_path(), build.kernel_resources_robust_path()):
        assert not [n for n in resources(path) if "lpe" in n.lower()], path
    src = open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_lpe.hip")).read()
    assert len(re.findall(r"__global__", src)) == 3 and "__shared__" not in src and "atomic" not in src.split("lpe_deposit_kernel:")[0]
