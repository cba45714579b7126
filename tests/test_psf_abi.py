"""The point-spread stage (vk_psf_*, additive symbols of ABI 7) on the CPU: the ten functions and the three debug hooks declared, exported
by both libraries, bound, declared in the Rust shim; the two structs' sizes and offsets as gcc lays them out against the ctypes mirror; no
stream-taking function; the defaults; the refusals that need no device, each leaving its outputs untouched; vk_psf_star's laws; the
kernels of vk_psf.hip in a resource record of their own — exactly the new ones, without scratch, AGPRs, spills or a dynamic stack, with
the LDS the line kernel was built with — and in none of the other ten."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_psf_default_params", "vk_psf_star", "vk_psf_create", "vk_psf_load", "vk_psf_load_device", "vk_psf_apply",
             "vk_psf_apply_device", "vk_psf_reset", "vk_psf_get_info", "vk_psf_destroy"]
HOOKS = ["vk_psf_debug_twiddles", "vk_psf_debug_fft2", "vk_psf_debug_last_pass_ms"]
STRUCTS = {"vk_psf_params": ffi.PsfParams, "vk_psf_info": ffi.PsfInfo}
SIZES = {"vk_psf_params": 20, "vk_psf_info": 64}
# name -> LDS bytes.  The line kernel: one row of up to 4096 complex values (8 bytes each), or a tile of adjacent columns of up to 8192.
KERNELS = {
    "_Z14psf_pad_kernel10PsfPadArgs": 0,
    "_Z16psf_place_kernel12PsfPlaceArgs": 0,
    "_Z17psf_bitrev_kernel12PsfStageArgs": 0,
    "_Z16psf_stage_kernel12PsfStageArgs": 0,
    "_Z18psf_product_kernel14PsfProductArgs": 0,
    "_Z16psf_scale_kernel12PsfScaleArgs": 0,
    "_Z20psf_composite_kernel16PsfCompositeArgs": 0,
    "_Z15psf_line_kernelILb0EEv11PsfLineArgs": 8 * 4096,
    "_Z15psf_line_kernelILb1EEv11PsfLineArgs": 8 * 8192,
}
OTHER_STAGES = r"adapt|splat|matte|robust|lpe|tone|nlm|glare|upsample"


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
    assert lib.vk_psf_create.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    assert lib.vk_psf_load.argtypes == lib.vk_psf_load_device.argtypes == [C.c_void_p, C.c_uint32, C.c_void_p]
    assert lib.vk_psf_apply.argtypes == lib.vk_psf_apply_device.argtypes == [C.c_void_p, C.POINTER(ffi.PsfParams), C.c_void_p, C.c_void_p]
    assert lib.vk_psf_get_info.argtypes == [C.c_void_p, C.POINTER(ffi.PsfInfo)]
    assert lib.vk_psf_destroy.restype is None and lib.vk_psf_destroy.argtypes == [C.c_void_p]
    assert lib.vk_psf_debug_fft2.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    assert all(getattr(lib, fn).restype is C.c_int for fn in FUNCTIONS[:-1] + HOOKS)
    assert re.search(r"enum \{ VK_PSF_FORM_AUTO = 0, VK_PSF_FORM_PLAIN = 1, VK_PSF_FORM_LDS = 2 \};", code(hdr))
    assert (ffi.VK_PSF_FORM_AUTO, ffi.VK_PSF_FORM_PLAIN, ffi.VK_PSF_FORM_LDS) == (0, 1, 2)
    # the names carry `psf` and none of the words other features' ABI tests look for
    for fn in FUNCTIONS + HOOKS:
        assert "psf" in fn and not re.search(OTHER_STAGES + "|denoise|temporal", fn), fn
    # the section's form: what it replaces, state, ordering, the operator, refusals
    sec = hdr[hdr.index("/* ---- point-spread function"):hdr.index("typedef struct vk_psf vk_psf;")]
    for word in ("replaces: nothing", "State.", "ENQUEUED on the null stream", "The operator, exactly.", "Twiddle tables", "What this is not.",
                 "VK_ERR_OOM leaves *out untouched"):
        assert word in sec, word
    p = ffi.PsfParams(9, 9, 9, 9, 9)
    assert lib.vk_psf_default_params(C.byref(p)) == ffi.VK_OK
    assert (np.float32(p.strength), p.threshold, p.form, p.flags, p._pad) == (np.float32(0.15), 0.0, ffi.VK_PSF_FORM_AUTO, 0, 0)


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    want = {
        "vk_psf_default_params": r"out: \*mut vk_psf_params\) -> c_int;",
        "vk_psf_star": r"K: u32, streaks: u32, rotation: f32, sharpness: f32, chroma: f32, out: \*mut f32\) -> c_int;",
        "vk_psf_create": r"scene: \*mut vk_scene, width: u32, height: u32, kmax: u32, out: \*mut \*mut vk_psf\) -> c_int;",
        "vk_psf_load": r"h: \*mut vk_psf, K: u32, kernel: \*const f32\) -> c_int;",
        "vk_psf_load_device": r"h: \*mut vk_psf, K: u32, d_kernel: \*const c_void\) -> c_int;",
        "vk_psf_apply": r"h: \*mut vk_psf, p: \*const vk_psf_params, rgb_in: \*const f32, rgb_out: \*mut f32\) -> c_int;",
        "vk_psf_apply_device": r"h: \*mut vk_psf, p: \*const vk_psf_params, d_rgb_in: \*const c_void, d_rgb_out: \*mut c_void\) -> c_int;",
        "vk_psf_reset": r"h: \*mut vk_psf\) -> c_int;",
        "vk_psf_get_info": r"h: \*mut vk_psf, out: \*mut vk_psf_info\) -> c_int;",
        "vk_psf_destroy": r"h: \*mut vk_psf\);",
    }
    assert sorted(want) == sorted(FUNCTIONS)
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    assert re.search(r"#\[repr\(C\)\] pub struct vk_psf \{ _private: \[u8; 0\] \}", rs)
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
    assert n == 5 + 12
    assert [f for f, _ in ffi.PsfParams._fields_] == ["strength", "threshold", "form", "flags", "_pad"]


def test_no_psf_function_takes_a_stream():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*psf\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args, fn
    assert seen == FUNCTIONS + HOOKS


def params(**kw):
    p = ffi.PsfParams(0.15, 0.0, 0, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


NAN, INF = float("nan"), float("inf")
REFUSALS = [(dict(strength=-0.01), b"strength must be in [0, 1]"), (dict(strength=1.01), b"strength must be in [0, 1]"),
            (dict(strength=NAN), b"strength must be in [0, 1]"), (dict(strength=INF), b"strength must be in [0, 1]"),
            (dict(threshold=-0.5), b"threshold must be finite and >= 0"), (dict(threshold=NAN), b"threshold must be finite and >= 0"),
            (dict(threshold=INF), b"threshold must be finite and >= 0"), (dict(form=3), b"unknown psf form"),
            (dict(form=0xFFFFFFFF), b"unknown psf form"), (dict(flags=1), b"unknown psf flags"), (dict(_pad=1), b"unknown psf flags")]


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    h = C.c_void_p(0x1000)                # never read: each of these is refused first
    out = C.c_void_p(0x77)
    assert lib.vk_psf_default_params(None) == ffi.VK_ERR_BAD_ARG
    for args in ((None, 4, 4, 3, C.byref(out)), (h, 4, 4, 3, None)):
        assert lib.vk_psf_create(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    for dims, word in (((0, 4, 3), b"width and height must be >= 1"), ((4, 0, 3), b"width and height must be >= 1"),
                       ((4, 4, 4), b"kmax must be odd and in 3..1023"), ((4, 4, 1), b"kmax must be odd and in 3..1023"),
                       ((4, 4, 1025), b"kmax must be odd and in 3..1023"), ((4095, 4, 3), b"padded size exceeds 4096"),
                       ((4, 4095, 3), b"padded size exceeds 4096"), ((3075, 4, 1023), b"padded size exceeds 4096"),
                       ((0xFFFFFFFF, 0xFFFFFFFF, 1023), b"padded size exceeds 4096")):
        assert lib.vk_psf_create(h, *dims, C.byref(out)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), dims
    assert out.value == 0x77
    src, dst = np.full(48, 7, np.float32), np.full(48, 7, np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    ok = params()
    for apply in (lib.vk_psf_apply, lib.vk_psf_apply_device):
        for args in ((None, C.byref(ok), p(src), p(dst)), (h, None, p(src), p(dst)), (h, C.byref(ok), None, p(dst)), (h, C.byref(ok), p(src), None)):
            assert apply(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
        for kw, word in REFUSALS:
            bad = params(**kw)
            assert apply(h, C.byref(bad), p(src), p(dst)) == ffi.VK_ERR_BAD_ARG, kw
            assert word in lib.vk_last_error(), (kw, lib.vk_last_error())
    assert (src == 7).all() and (dst == 7).all()
    for load in (lib.vk_psf_load, lib.vk_psf_load_device):
        assert load(None, 3, p(src)) == ffi.VK_ERR_BAD_ARG and load(h, 3, None) == ffi.VK_ERR_BAD_ARG
        for K in (0, 1, 2, 4, 1024, 1025, 0xFFFFFFFF):
            assert load(h, K, p(src)) == ffi.VK_ERR_BAD_ARG and b"K must be odd and in 3..1023" in lib.vk_last_error(), K
    canary = ffi.PsfInfo(9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9.0, 9)
    info = ffi.PsfInfo.from_buffer_copy(canary)
    assert lib.vk_psf_get_info(None, C.byref(info)) == ffi.VK_ERR_BAD_ARG and lib.vk_psf_get_info(h, None) == ffi.VK_ERR_BAD_ARG
    assert bytes(info) == bytes(canary)
    assert lib.vk_psf_reset(None) == ffi.VK_ERR_BAD_ARG
    ms = (C.c_double * 4)(7, 7, 7, 7)
    assert lib.vk_psf_debug_last_pass_ms(None, C.byref(ms)) == ffi.VK_ERR_BAD_ARG and lib.vk_psf_debug_last_pass_ms(h, None) == ffi.VK_ERR_BAD_ARG
    assert list(ms) == [7, 7, 7, 7]
    lib.vk_psf_destroy(None)              # nothing
    T = np.full(8, 7, np.float32)
    assert lib.vk_psf_debug_twiddles(8, None) == ffi.VK_ERR_BAD_ARG
    for N in (0, 1, 3, 6, 8192):
        assert lib.vk_psf_debug_twiddles(N, p(T)) == ffi.VK_ERR_BAD_ARG, N
    assert (T == 7).all()
    assert lib.vk_psf_debug_twiddles(8, p(T)) == ffi.VK_OK and T[0] == 1 and T[1] == 0 and T[4] == 0 and T[5] == -1
    for args in ((None, 4, 4, 0, 1, p(src)), (h, 4, 4, 0, 1, None), (h, 3, 4, 0, 1, p(src)), (h, 4, 8192, 0, 1, p(src)), (h, 4, 1, 0, 1, p(src)),
                 (h, 4, 4, 2, 1, p(src)), (h, 4, 4, 0, 0, p(src)), (h, 4, 4, 0, 3, p(src))):
        assert lib.vk_psf_debug_fft2(*args) == ffi.VK_ERR_BAD_ARG, args[1:5]
    assert (src == 7).all()


def star(K, streaks, rotation=0.0, sharpness=8.0, chroma=0.0):
    lib = ffi.load_device_lib()
    out = np.full((K, K, 3), 7, np.float32)
    assert lib.vk_psf_star(K, streaks, rotation, sharpness, chroma, C.c_void_p(out.ctypes.data)) == ffi.VK_OK, lib.vk_last_error()
    return out


def test_the_star(built):
    lib = ffi.load_device_lib()
    out = np.full((5, 5, 3), 7, np.float32)
    ptr = C.c_void_p(out.ctypes.data)
    assert lib.vk_psf_star(5, 6, 0.0, 8.0, 0.0, None) == ffi.VK_ERR_BAD_ARG
    for args in ((4, 6, 0.0, 8.0, 0.0), (1, 6, 0.0, 8.0, 0.0), (1025, 6, 0.0, 8.0, 0.0), (5, 65, 0.0, 8.0, 0.0), (5, 6, NAN, 8.0, 0.0),
                 (5, 6, 0.0, 0.5, 0.0), (5, 6, 0.0, NAN, 0.0), (5, 6, 0.0, 8.0, -0.1), (5, 6, 0.0, 8.0, 0.6), (5, 6, 0.0, 8.0, NAN)):
        assert lib.vk_psf_star(*args, ptr) == ffi.VK_ERR_BAD_ARG, args
    assert (out == 7).all()
    for K, streaks, chroma in ((3, 0, 0.0), (65, 6, 0.0), (65, 4, 0.15), (129, 8, 0.3)):
        k = star(K, streaks, 0.3, 8.0, chroma)
        assert np.isfinite(k).all() and (k >= 0).all()
        # each tap is (float)(v / S): K * K roundings of at most half an ulp of a value below 1
        assert (np.abs(k.astype(np.float64).sum(axis=(0, 1)) - 1.0) <= K * K * 2.0 ** -25).all(), (K, streaks)
        if chroma == 0.0:
            assert np.array_equal(k[..., 0], k[..., 1]) and np.array_equal(k[..., 1], k[..., 2])
        else:
            assert not np.array_equal(k[..., 0], k[..., 1]) and not np.array_equal(k[..., 1], k[..., 2])
            # a larger radial scale spreads wider: the centre tap holds less of the channel
            r = (K - 1) // 2
            assert k[r, r, 0] > k[r, r, 1] > k[r, r, 2]
    # the formula, in f64: within the final f32 rounding and libm's last bits
    K, n, rot, sh, ch = 33, 6, 0.2, 4.0, 0.1
    k = star(K, n, rot, sh, ch)
    r = (K - 1) // 2
    y, x = np.mgrid[-r:r + 1, -r:r + 1].astype(np.float64)
    for c in range(3):
        g = 1.0 + float(np.float32(ch)) * (c - 1)
        d = np.sqrt(x * x + y * y) / g
        v = np.exp(-0.5 * d * d)
        ray = 0.25 * np.abs(np.cos(0.5 * n * (np.arctan2(y, x) - float(np.float32(rot))))) ** sh * (1.0 - d / r) ** 2 / (1.0 + d)
        v = v + np.where((d > 0) & (d < r), ray, 0.0)
        want = v / v.sum()
        assert np.abs(k[..., c] - want).max() <= 2.0 ** -24 * want.max() + 1e-12, c
    # Invariant under a rotation by one streak spacing.  The rays' term has that period exactly, so the two kernels differ by the rounding
    # of the rotation to the f32 the call takes: half an ulp of a value below 4, 2^-23; 2^-22 with libm's last bits.  Inside the cosine
    # that is streaks / 2 times as much, |cos|^sharpness has slope at most sharpness, and the ray's factor is at most 0.25: a tap's
    # unnormalised value moves by at most delta.  Normalised, a = v / S with S >= 1 (the centre's core): |a - a'| <= delta / S + a' *
    # (K * K * delta) / S <= delta * (1 + K * K * max(a)).  Then the two f32 roundings.
    K, sharp = 33, 8.0
    for n in (4, 6, 7):
        a, b = star(K, n, 0.1, sharp, 0.0), star(K, n, 0.1 + 2 * math.pi / n, sharp, 0.0)
        delta = 0.25 * sharp * (n / 2) * 2.0 ** -22
        tol = delta * (1 + K * K * float(a.max())) + 2.0 ** -23
        assert np.abs(a.astype(np.float64) - b).max() <= tol, (n, np.abs(a.astype(np.float64) - b).max(), tol)
        assert np.abs(a - star(K, n, 0.1 + math.pi / n, sharp, 0.0)).max() > 10 * tol      # half a spacing is another kernel


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
    """kernel_resources_psf.txt lists exactly the kernels of vk_psf.hip, each once: no scratch, no scratch instructions, no AGPRs, no
    spills, no dynamic stack; the line kernel's LDS, at most 64 KB; the other ten records and vk_kernels.h hold none of them, and the
    names hold no other stage's word"""
    mine = resources(build.kernel_resources_psf_path())
    assert sorted(mine) == sorted(KERNELS), sorted(mine)
    for name, r in mine.items():
        assert r["agprs"] == 0 and r["scratch"] == 0 and r["scratch_ops"] == 0 and r["spills"] == 0 and r["sgpr_spills"] == 0, (name, r)
        assert not r["dynamic_stack"], name
        assert r["lds"] == KERNELS[name] and r["lds"] <= 65536, (name, r)
        assert r["vgprs"] <= 64 and r["occupancy"] >= (8 if r["lds"] == 0 else 2), (name, r)
        assert not re.search(OTHER_STAGES, name.lower()), name
    others = (build.kernel_resources_path(), build.kernel_resources_adapt_path(), build.kernel_resources_splat_path(),
              build.kernel_resources_matte_path(), build.kernel_resources_robust_path(), build.kernel_resources_lpe_path(),
              build.kernel_resources_tone_path(), build.kernel_resources_nlm_path(), build.kernel_resources_glare_path(),
              build.kernel_resources_upsample_path())
    assert len(others) == 10
    for path in others:
        assert "psf" not in open(path).read().lower(), path
    src = open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_psf.hip")).read()
    assert len(re.findall(r"__global__", src)) == 8 and "asm" not in src
    assert "asm" not in open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_psf.h")).read()
    assert "psf" not in open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_kernels.h")).read().lower()
