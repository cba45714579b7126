"""Display transform (vk_tone_*, additive symbols of ABI 7) on the CPU: the twelve functions and the four debug hooks declared, exported
by both libraries, bound, declared in the Rust shim; the four structs' sizes and offsets as gcc lays them out against the ctypes mirror;
no stream-taking function; the refusals that need no device, each leaving its outputs untouched; the two tables (strictly increasing,
each entry the smallest f32 not below the test's own f64 value, up to one ulp); the kernels of vk_tone.hip in a resource record of
their own — exactly the new ones, without scratch, AGPRs or a dynamic stack, with the LDS each form was built with — and in none of the
other six."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import tone_ref as T
from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["vk_tone_default_meter_params", "vk_tone_default_params", "vk_tone_create", "vk_tone_load", "vk_tone_load_device",
             "vk_tone_meter", "vk_tone_solve", "vk_tone_encode", "vk_tone_encode_device", "vk_tone_reset", "vk_tone_get_info",
             "vk_tone_destroy"]
HOOKS = ["vk_debug_tone_histogram", "vk_debug_tone_table", "vk_debug_tone_set_form", "vk_debug_tone_last_ms"]
STRUCTS = {"vk_tone_meter_params": ffi.ToneMeterParams, "vk_tone_meter_info": ffi.ToneMeterInfo, "vk_tone_params": ffi.ToneParams,
           "vk_tone_info": ffi.ToneInfo}
SIZES = {"vk_tone_meter_params": 32, "vk_tone_meter_info": 56, "vk_tone_params": 32, "vk_tone_info": 48}
METERS = {"_Z21tone_meter_lds_kernel13ToneMeterArgs": 2560, "_Z23tone_meter_plain_kernel13ToneMeterArgs": 0}
ENCODES = {f"_Z18tone_encode_kernelILj{c}ELb{t}ELb{d}EEv14ToneEncodeArgs": 2040 * t for c in range(4) for t, d in ((0, 0), (1, 0), (1, 1))}


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
    assert lib.vk_tone_create.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    assert lib.vk_tone_meter.argtypes == [C.c_void_p, C.POINTER(ffi.ToneMeterParams), C.POINTER(ffi.ToneMeterInfo)]
    assert lib.vk_tone_solve.argtypes == [C.c_void_p, C.POINTER(ffi.ToneMeterParams), C.POINTER(C.c_double), C.POINTER(ffi.ToneMeterInfo)]
    assert lib.vk_tone_encode.argtypes == lib.vk_tone_encode_device.argtypes == [C.c_void_p, C.POINTER(ffi.ToneParams), C.c_void_p]
    assert lib.vk_tone_load.argtypes == lib.vk_tone_load_device.argtypes == [C.c_void_p, C.c_void_p]
    assert lib.vk_tone_get_info.argtypes == [C.c_void_p, C.POINTER(ffi.ToneInfo)]
    assert lib.vk_tone_destroy.restype is None and lib.vk_tone_destroy.argtypes == [C.c_void_p]
    assert lib.vk_debug_tone_last_ms.argtypes == [C.c_void_p, C.POINTER(C.c_double * 2)]
    assert all(getattr(lib, fn).restype is C.c_int for fn in FUNCTIONS[:-1] + HOOKS)
    for line, names in ((r"enum \{ VK_TONE_CLAMP = 0, VK_TONE_REINHARD = 1, VK_TONE_HABLE = 2, VK_TONE_ACES = 3 \};", T.CURVES),
                        (r"enum \{ VK_TONE_TRANSFER_REFERENCE = 0, VK_TONE_TRANSFER_SRGB = 1, VK_TONE_TRANSFER_GAMMA22 = 2 \};", T.TRANSFERS)):
        assert re.search(line, code(hdr)) and tuple(names) == tuple(range(len(names)))
    assert re.search(r"enum \{ VK_TONE_USE_METERED = 1, VK_TONE_DITHER = 2 \};", code(hdr)) and re.search(r"enum \{ VK_TONE_METER_EMPTY = 1 \};", code(hdr))
    assert (ffi.VK_TONE_USE_METERED, ffi.VK_TONE_DITHER, ffi.VK_TONE_METER_EMPTY, ffi.VK_TONE_FORM_LDS, ffi.VK_TONE_FORM_PLAIN) == (1, 2, 1, 0, 1)
    mp = ffi.ToneMeterParams(9, 9, 9, 9, 9, 9, (9, 9))
    assert lib.vk_tone_default_meter_params(C.byref(mp)) == ffi.VK_OK
    f32 = np.float32
    assert (f32(mp.key), f32(mp.low_fraction), f32(mp.high_fraction), mp.blend, mp.min_log2, mp.max_log2, list(mp._pad)) == \
        (f32(0.18), f32(0.10), f32(0.02), 1.0, -16.0, 16.0, [0, 0])
    tp = ffi.ToneParams(9, 9, 9, 9, 9, 9, 9)
    assert lib.vk_tone_default_params(C.byref(tp)) == ffi.VK_OK
    assert (tp.curve, tp.transfer, tp.flags, tp._pad, tp.exposure, f32(tp.white), tp.seed) == \
        (ffi.VK_TONE_ACES, ffi.VK_TONE_TRANSFER_SRGB, ffi.VK_TONE_USE_METERED, 0, 1.0, f32(11.2), 0)


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    want = {
        "vk_tone_default_meter_params": r"out: \*mut vk_tone_meter_params\) -> c_int;",
        "vk_tone_default_params": r"out: \*mut vk_tone_params\) -> c_int;",
        "vk_tone_create": r"scene: \*mut vk_scene, width: u32, height: u32, out: \*mut \*mut vk_tone\) -> c_int;",
        "vk_tone_load": r"t: \*mut vk_tone, rgb: \*const f32\) -> c_int;",
        "vk_tone_load_device": r"t: \*mut vk_tone, d_rgb: \*const c_void\) -> c_int;",
        "vk_tone_meter": r"t: \*mut vk_tone, mp: \*const vk_tone_meter_params, out: \*mut vk_tone_meter_info\) -> c_int;",
        "vk_tone_solve": r"bins: \*const u32, mp: \*const vk_tone_meter_params, prev_log2: \*const f64, out: \*mut vk_tone_meter_info\) -> c_int;",
        "vk_tone_encode": r"t: \*mut vk_tone, tp: \*const vk_tone_params, rgb8_out: \*mut u8\) -> c_int;",
        "vk_tone_encode_device": r"t: \*mut vk_tone, tp: \*const vk_tone_params, d_rgb8_out: \*mut c_void\) -> c_int;",
        "vk_tone_reset": r"t: \*mut vk_tone\) -> c_int;",
        "vk_tone_get_info": r"t: \*mut vk_tone, out: \*mut vk_tone_info\) -> c_int;",
        "vk_tone_destroy": r"t: \*mut vk_tone\);",
    }
    assert sorted(want) == sorted(FUNCTIONS)
    for fn, args in want.items():
        assert re.search(r"pub fn " + fn + r"\(" + args, rs), fn
    assert re.search(r"#\[repr\(C\)\] pub struct vk_tone \{ _private: \[u8; 0\] \}", rs)
    consts = {"VK_TONE_CLAMP": 0, "VK_TONE_REINHARD": 1, "VK_TONE_HABLE": 2, "VK_TONE_ACES": 3, "VK_TONE_TRANSFER_REFERENCE": 0,
              "VK_TONE_TRANSFER_SRGB": 1, "VK_TONE_TRANSFER_GAMMA22": 2, "VK_TONE_USE_METERED": 1, "VK_TONE_DITHER": 2, "VK_TONE_METER_EMPTY": 1}
    assert all(re.search(rf"pub const {n}: u32 = {v};", rs) for n, v in consts.items())
    import test_rust_shim_layout as R
    c, r = R.c_structs(), R.rust_structs()
    for name in STRUCTS:
        assert name in c and r.get(name) == c[name], name
    assert ("_pad", "[u32; 2]") in c["vk_tone_meter_params"]


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """the four structs' sizes, and every field's offset and size: the header through gcc against ctypes"""
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
    assert n == 7 + 8 + 7 + 8
    assert [f for f, _ in ffi.ToneMeterParams._fields_] == ["key", "low_fraction", "high_fraction", "blend", "min_log2", "max_log2", "_pad"]
    assert [f for f, _ in ffi.ToneParams._fields_] == ["curve", "transfer", "flags", "_pad", "exposure", "white", "seed"]


def test_no_tone_function_takes_a_stream():
    seen = []
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        for fn, args in re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*tone\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            seen.append(fn)
            assert "stream" not in args, fn
    assert seen == FUNCTIONS + HOOKS


def meter_params(**kw):
    mp = ffi.ToneMeterParams(0.18, 0.10, 0.02, 1.0, -16.0, 16.0, (0, 0))
    for k, v in kw.items():
        setattr(mp, k, v)
    return mp


def tone_params(**kw):
    tp = ffi.ToneParams(ffi.VK_TONE_ACES, ffi.VK_TONE_TRANSFER_SRGB, 0, 0, 1.0, 11.2, 0)
    for k, v in kw.items():
        setattr(tp, k, v)
    return tp


METER_REFUSALS = [(dict(_pad=(0, 1)), b"_pad must be 0"), (dict(_pad=(7, 0)), b"_pad must be 0"),
                  (dict(low_fraction=-0.01), b"must be finite and >= 0"), (dict(high_fraction=-1.0), b"must be finite and >= 0"),
                  (dict(low_fraction=float("nan")), b"must be finite and >= 0"), (dict(high_fraction=float("inf")), b"must be finite and >= 0"),
                  (dict(low_fraction=0.5, high_fraction=0.5), b"must be below 1"), (dict(low_fraction=1.0, high_fraction=0.0), b"must be below 1"),
                  (dict(key=0.0), b"key must be finite and > 0"), (dict(key=-1.0), b"key must be finite and > 0"),
                  (dict(key=float("inf")), b"key must be finite and > 0"), (dict(key=float("nan")), b"key must be finite and > 0"),
                  (dict(blend=-0.1), b"blend must be in 0..1"), (dict(blend=1.5), b"blend must be in 0..1"),
                  (dict(blend=float("nan")), b"blend must be in 0..1"),
                  (dict(min_log2=float("nan")), b"must be finite and within"), (dict(max_log2=float("inf")), b"must be finite and within"),
                  (dict(min_log2=-2000.0), b"must be finite and within"),
                  (dict(min_log2=2.0, max_log2=1.0), b"min_log2 must not exceed max_log2")]
ENCODE_REFUSALS = [(dict(_pad=1), b"_pad must be 0"), (dict(curve=4), b"unknown curve"), (dict(curve=0xFFFFFFFF), b"unknown curve"),
                   (dict(transfer=3), b"unknown transfer"), (dict(flags=4), b"unknown tone flags"),
                   (dict(flags=ffi.VK_TONE_DITHER, transfer=ffi.VK_TONE_TRANSFER_REFERENCE), b"dither needs a table transfer"),
                   (dict(exposure=0.0), b"exposure must be finite and > 0"), (dict(exposure=float("inf")), b"exposure must be finite and > 0"),
                   (dict(exposure=float("nan")), b"exposure must be finite and > 0"), (dict(exposure=-2.0), b"exposure must be finite and > 0"),
                   (dict(white=0.0), b"white must be finite and > 0"), (dict(white=float("nan")), b"white must be finite and > 0"),
                   (dict(white=float("inf")), b"white must be finite and > 0"),                      # ACES: +inf is REINHARD's alone
                   (dict(white=float("inf"), curve=ffi.VK_TONE_HABLE), b"white must be finite and > 0"),
                   (dict(white=float("-inf"), curve=ffi.VK_TONE_REINHARD), b"white must be finite and > 0")]


def test_refusals_that_need_no_device(built):
    lib = ffi.load_device_lib()
    h = C.c_void_p(0x1000)                # never read: each of these is refused first
    out = C.c_void_p(0x77)
    assert lib.vk_tone_default_meter_params(None) == ffi.VK_ERR_BAD_ARG and lib.vk_tone_default_params(None) == ffi.VK_ERR_BAD_ARG
    for args in ((None, 4, 4, C.byref(out)), (h, 4, 4, None)):
        assert lib.vk_tone_create(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    for dims, word in (((0, 4), b"width and height must be >= 1"), ((4, 0), b"width and height must be >= 1"),
                       ((16385, 8192), b"width * height exceeds 2^27"), ((0xFFFFFFFF, 0xFFFFFFFF), b"exceeds 2^27")):
        assert lib.vk_tone_create(h, *dims, C.byref(out)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), dims
    assert out.value == 0x77
    # the solve: nulls, every bad field, a non-finite previous exposure; the info stays as it was
    bins = np.zeros(640, np.uint32)
    bins[300] = 5
    canary = ffi.ToneMeterInfo(9.0, 9.0, 9, 9, 9, 9, 9.0, 9)
    info = ffi.ToneMeterInfo.from_buffer_copy(canary)
    ok = meter_params()
    for args in ((None, C.byref(ok), None, C.byref(info)), (bins.ctypes.data, None, None, C.byref(info)), (bins.ctypes.data, C.byref(ok), None, None)):
        assert lib.vk_tone_solve(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    for kw, word in METER_REFUSALS:
        bad = meter_params(**kw)
        assert lib.vk_tone_solve(bins.ctypes.data, C.byref(bad), None, C.byref(info)) == ffi.VK_ERR_BAD_ARG, kw
        assert word in lib.vk_last_error(), (kw, lib.vk_last_error())
        # (the handle is never read: the parameters are refused first)
        assert lib.vk_tone_meter(h, C.byref(bad), C.byref(info)) == ffi.VK_ERR_BAD_ARG and word in lib.vk_last_error(), kw
    for prev in (float("nan"), float("inf")):
        p = C.c_double(prev)
        assert lib.vk_tone_solve(bins.ctypes.data, C.byref(ok), C.byref(p), C.byref(info)) == ffi.VK_ERR_BAD_ARG
        assert b"prev_log2 must be finite" in lib.vk_last_error()
    assert bytes(info) == bytes(canary)
    # the fractions may add up to just below 1, and the solve then succeeds without a device
    assert lib.vk_tone_solve(bins.ctypes.data, C.byref(meter_params(low_fraction=0.5, high_fraction=0.49)), None, C.byref(info)) == ffi.VK_OK
    assert info.binned == 5 and info.flags == 0
    # meter, load, encode: nulls
    assert lib.vk_tone_meter(None, C.byref(ok), C.byref(info)) == ffi.VK_ERR_BAD_ARG and lib.vk_tone_meter(h, None, C.byref(info)) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_tone_meter(h, C.byref(ok), None) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    img = np.full(48, 7, np.float32)
    for load in (lib.vk_tone_load, lib.vk_tone_load_device):
        assert load(None, img.ctypes.data) == ffi.VK_ERR_BAD_ARG and load(h, None) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
    codes = np.full(48, 7, np.uint8)
    tp = tone_params()
    for enc in (lib.vk_tone_encode, lib.vk_tone_encode_device):
        for args in ((None, C.byref(tp), codes.ctypes.data), (h, None, codes.ctypes.data), (h, C.byref(tp), None)):
            assert enc(*args) == ffi.VK_ERR_BAD_ARG and b"null argument" in lib.vk_last_error()
        for kw, word in ENCODE_REFUSALS:
            bad = tone_params(**kw)
            assert enc(h, C.byref(bad), codes.ctypes.data) == ffi.VK_ERR_BAD_ARG, kw
            assert word in lib.vk_last_error(), (kw, lib.vk_last_error())
    assert (codes == 7).all() and (img == 7).all()
    assert lib.vk_tone_reset(None) == ffi.VK_ERR_BAD_ARG and b"null tone handle" in lib.vk_last_error()
    ti = ffi.ToneInfo(9, 9, 9, 9, 9, 9.0, 9, 9.0)
    assert lib.vk_tone_get_info(None, C.byref(ti)) == ffi.VK_ERR_BAD_ARG and lib.vk_tone_get_info(h, None) == ffi.VK_ERR_BAD_ARG
    assert bytes(ti) == bytes(ffi.ToneInfo(9, 9, 9, 9, 9, 9.0, 9, 9.0))
    lib.vk_tone_destroy(None)             # nothing
    hb, hc = np.full(640, 7, np.uint32), np.full(4, 7, np.uint64)
    for args in ((None, hb.ctypes.data, hc.ctypes.data), (h, None, hc.ctypes.data), (h, hb.ctypes.data, None)):
        assert lib.vk_debug_tone_histogram(*args) == ffi.VK_ERR_BAD_ARG
    tab = np.full(510, 7, np.float32)
    assert lib.vk_debug_tone_table(ffi.VK_TONE_TRANSFER_SRGB, None) == ffi.VK_ERR_BAD_ARG
    for transfer in (ffi.VK_TONE_TRANSFER_REFERENCE, 3, 0xFFFFFFFF):
        assert lib.vk_debug_tone_table(transfer, tab.ctypes.data) == ffi.VK_ERR_BAD_ARG and b"not a table transfer" in lib.vk_last_error()
    assert lib.vk_debug_tone_set_form(None, 0) == ffi.VK_ERR_BAD_ARG
    ms = (C.c_double * 2)(7, 7)
    assert lib.vk_debug_tone_last_ms(None, C.byref(ms)) == ffi.VK_ERR_BAD_ARG and lib.vk_debug_tone_last_ms(h, None) == ffi.VK_ERR_BAD_ARG
    assert list(ms) == [7, 7] and (hb == 7).all() and (hc == 7).all() and (tab == 7).all()


def library_table(transfer):
    tab = np.full(512, 7, np.float32)
    assert ffi.load_device_lib().vk_debug_tone_table(transfer, tab[1:].ctypes.data) == ffi.VK_OK
    assert tab[0] == 7 and tab[511] == 7                      # 510 floats, no more
    return tab[1:511].copy()


def test_the_tables(built):
    """contract 5: strictly increasing; each entry not below the test's own f64 value and within one f32 ulp of it; H[510] = 1; needs
    no device"""
    for transfer in (T.SRGB, T.GAMMA22):
        tab = library_table(transfer)
        want = T.table64(transfer)
        assert (np.diff(tab.astype(np.float64)) > 0).all(), transfer
        below = np.nextafter(tab, np.float32(-np.inf))
        assert (tab.astype(np.float64) >= want).all(), transfer                                          # not below
        assert (below.astype(np.float64) < want).all(), transfer                                         # within one ulp: the smallest such
        assert tab[509] == 1.0 and tab[0] > 0
    srgb = library_table(T.SRGB)
    assert srgb[0] == np.float32(1.0 / 510.0 / 12.92) or srgb[0] == np.nextafter(np.float32(1.0 / 510.0 / 12.92), np.float32(1))


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
    """kernel_resources_tone.txt lists exactly the kernels of vk_tone.hip, each once — the two meter forms and one encode per (curve,
    reference or table, dither) —: no scratch, no AGPRs, no dynamic stack; the meter's LDS form holds its 640 bins (2560 bytes), the
    plain form nothing; the table instances of the encode hold the 510 thresholds (2040 bytes), the reference instances nothing; the
    other six records hold none of them"""
    mine = resources(build.kernel_resources_tone_path())
    want = {**METERS, **ENCODES}
    assert len(ENCODES) == 12 and sorted(mine) == sorted(want), sorted(mine)
    for name, r in mine.items():
        assert r["agprs"] == 0 and r["scratch"] == 0 and r["scratch_ops"] == 0 and not r["dynamic_stack"], (name, r)
        assert r["lds"] == want[name] and r["vgprs"] <= 64 and r["occupancy"] == 8, (name, r)
    for path in (build.kernel_resources_path(), build.kernel_resources_adapt_path(), build.kernel_resources_splat_path(),
                 build.kernel_resources_matte_path(), build.kernel_resources_robust_path(), build.kernel_resources_lpe_path()):
        assert "tone" not in open(path).read().lower(), path
    src = open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_tone.hip")).read()
    assert len(re.findall(r"__global__", src)) == 3 and "asm" not in src
    assert "tone" not in open(os.path.join(ROOT, "vecchio_amd", "csrc", "vk_kernels.h")).read().lower()
