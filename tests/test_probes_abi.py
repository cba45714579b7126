"""Probe queries (vk_trace_probes, vk_probe_eval: additive symbols of ABI 7) on the CPU: declared, exported by both libraries, bound,
declared in the Rust shim; host-pointer entry points only; every argument vk_trace_radiance refuses, refused by both new calls without a
device and in the same words; probe_kernel's instances exist beside radiance_kernel's and gather_kernel's; vk_probe_eval against closed
forms."""
import ctypes as C
import os
import re

import numpy as np

from vecchio_amd import build, ffi
from vecchio_amd.scene import RAY_DTYPE, make_probes, probe_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC_ARGTYPES = [C.c_void_p, C.POINTER(ffi.RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(ffi.Stats)]
HOOK_ARGTYPES = [C.c_void_p, C.POINTER(ffi.RadianceParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(ffi.Stats)]


def headers():
    return [re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", f)).read(), flags=re.S)
            for f in ("vecchio_amd.h", "vecchio_amd_debug.h")]


def test_declared_exported_and_bound(built):
    hdr, dbg = headers()
    assert re.search(r"#define VK_ABI_VERSION 7\b", hdr) and re.search(r"#define VK_PROBE_COEFFS 9u\b", hdr)
    assert re.search(r"\bint vk_trace_probes\s*\(", hdr) and re.search(r"\bint vk_probe_eval\s*\(", hdr)
    assert re.search(r"\bint vk_debug_trace_probe_samples\s*\(", dbg)
    for path in (ffi.device_lib_path(), build.build_device_debug()):
        lib = C.CDLL(path)
        assert hasattr(lib, "vk_trace_probes") and hasattr(lib, "vk_probe_eval") and hasattr(lib, "vk_debug_trace_probe_samples"), path
        assert not hasattr(lib, "vk_trace_probes_device"), path
    assert "vk_trace_probes" in ffi.DEVICE_SYMBOLS and "vk_probe_eval" in ffi.DEVICE_SYMBOLS and ffi.VK_PROBE_COEFFS == 9
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    assert re.search(r"pub fn vk_trace_probes\(", rs) and re.search(r"pub fn vk_probe_eval\(", rs)
    assert re.search(r"pub const VK_PROBE_COEFFS: u32 = 9;", rs)
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == 7
    assert lib.vk_trace_probes.argtypes == PUBLIC_ARGTYPES and lib.vk_trace_probes.restype is C.c_int
    assert lib.vk_debug_trace_probe_samples.argtypes == HOOK_ARGTYPES and lib.vk_debug_trace_probe_samples.restype is C.c_int


def test_host_pointer_entry_points_only_and_no_radiance_in_a_name():
    """no function of either header whose name contains `probe` takes a stream, and none is named after the two other path queries (whose
    ABI tests enumerate such names)"""
    seen = []
    for text in headers():
        for m in re.finditer(r"\b(vk_\w*probe\w*)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
            seen.append(m.group(1))
            assert "stream" not in m.group(2).lower(), m.group(0)
            assert not m.group(1).endswith("_device") and "radiance" not in m.group(1), m.group(1)
    assert sorted(seen) == ["vk_debug_trace_probe_samples", "vk_probe_eval", "vk_trace_probes"], seen


def params(**over):
    kw = dict(seed=1, first_index=0, samples_per_ray=4, first_sample=0, max_depth=5, integrator=ffi.VK_INTEGRATOR_SCATTER,
              background=ffi.VK_BACKGROUND_SKY, background_color=ffi.F3(0, 0, 0), flags=0, _pad=0)
    kw.update(over)
    return ffi.RadianceParams(**kw)


def test_bad_arguments_refused_without_a_device_in_the_radiance_querys_words(built):
    lib = ffi.load_device_lib()
    rp = params()
    pts = np.zeros(4, RAY_DTYPE)
    rgb = np.full((4, 3), 7.0, np.float32)
    sh = np.full((4, 9, 3), 7.0, np.float32)
    samples = np.full((4, 4, 4), 7.0, np.float32)
    dirs = np.full((4, 4, 4), 7.0, np.float32)
    st = ffi.Stats()
    st.samples = 99
    scene = C.c_void_p(0x1000)            # never read: each of these is refused first
    r, o, h, s, d = pts.ctypes.data, rgb.ctypes.data, sh.ctypes.data, samples.ctypes.data, dirs.ctypes.data
    cases = [                              # (tests/test_radiance_abi.py's list)
        ((None, C.byref(rp), r, 4), b"null argument"),
        ((scene, None, r, 4), b"null argument"),
        ((scene, C.byref(rp), None, 4), b"null rays or output"),
        ((scene, C.byref(rp), r, 2 ** 32 + 1), b"2^32"),
        ((scene, C.byref(params(flags=1)), r, 4), b"flags"),
        ((scene, C.byref(params(samples_per_ray=0)), r, 4), b"samples_per_ray"),
        ((scene, C.byref(params(samples_per_ray=2 ** 26 + 1)), r, 4), b"samples_per_ray"),
        ((scene, C.byref(params(samples_per_ray=4, first_sample=2 ** 32 - 4)), r, 4), b"first_sample"),
        ((scene, C.byref(params(integrator=2)), r, 4), b"integrator"),
        ((scene, C.byref(params(background=2)), r, 4), b"background"),
    ]
    for args, word in cases:
        assert lib.vk_trace_radiance(*args, o, C.byref(st)) == ffi.VK_ERR_BAD_ARG, word
        said = lib.vk_last_error()
        assert word in said, said
        assert lib.vk_trace_probes(*args, h, C.byref(st)) == ffi.VK_ERR_BAD_ARG, word
        assert lib.vk_last_error() == said, (lib.vk_last_error(), said)
        assert lib.vk_debug_trace_probe_samples(*args, s, d, C.byref(st)) == ffi.VK_ERR_BAD_ARG, word
        assert lib.vk_last_error() == said, (lib.vk_last_error(), said)
    assert lib.vk_trace_probes(scene, C.byref(rp), r, 4, None, C.byref(st)) == ffi.VK_ERR_BAD_ARG
    assert b"null rays or output" in lib.vk_last_error()
    assert lib.vk_debug_trace_probe_samples(scene, C.byref(rp), r, 4, None, d, C.byref(st)) == ffi.VK_ERR_BAD_ARG
    # first_sample + samples_per_ray = 2^32 - 1 is the last window that is accepted (refused here for another reason only: flags)
    assert lib.vk_trace_probes(scene, C.byref(params(samples_per_ray=4, first_sample=2 ** 32 - 5, flags=1)), r, 4, h, C.byref(st)) == \
        ffi.VK_ERR_BAD_ARG and b"flags" in lib.vk_last_error()
    # outputs untouched
    assert st.samples == 99 and (sh == 7.0).all() and (samples == 7.0).all() and (dirs == 7.0).all()
    # no probes: VK_OK, nothing done, also with null arrays (the scene handle is not read)
    assert lib.vk_trace_probes(scene, C.byref(rp), None, 0, None, C.byref(st)) == ffi.VK_OK and st.samples == 0
    assert lib.vk_debug_trace_probe_samples(scene, C.byref(rp), None, 0, None, None, None) == ffi.VK_OK


def kernels(txt, pattern):
    seen = {}
    for blk in txt.split("Name: ")[1:]:
        m = re.search(pattern, blk.split("\n")[0])
        if m:
            get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
            seen[int(m.group(1))] = dict(minw=int(m.group(2)), vgprs=get("VGPRs"), agprs=get("AGPRs"), occupancy=get("Occupancy [waves/SIMD]"),
                                         static_lds=get("LDS Size [bytes/block]"), dynamic_stack="Dynamic Stack: True" in blk,
                                         scratch=get("ScratchSize [bytes/lane]"), scratch_ops=get("ScratchOps"))
    return seen


def test_probe_kernel_has_its_instances_beside_the_other_two(built):
    """probe_kernel<F, MINW>: sphere-only worlds, Cornell-type worlds and everything, each with and without the PDF integrator, at the
    wave counts radiance_kernel's instances are built for"""
    txt = open(build.kernel_resources_path()).read()
    seen = kernels(txt, r"12probe_kernelILj(\d+)ELi(\d+)EEEv")
    cornell = 0x2 | 0x4 | 0x10 | 0x100
    assert set(seen) == {0, 0x80, cornell, cornell | 0x80, 0x17F, 0x17F | 0x80}, sorted(seen)
    rad = kernels(txt, r"15radiance_kernelILj(\d+)ELi(\d+)EEEv")
    gat = kernels(txt, r"13gather_kernelILj(\d+)ELi(\d+)EEEv")
    assert set(rad) == set(seen) == set(gat)
    for F, r in seen.items():
        assert r["occupancy"] >= r["minw"] and r["agprs"] == 0 and r["static_lds"] == 0 and not r["dynamic_stack"], (F, r)
        assert r["minw"] == rad[F]["minw"], (F, r, rad[F])
        print(f"\n   probe_kernel<{F:#05x}, {r['minw']}>: {r['vgprs']} VGPRs, scratch {r['scratch']} B/lane in {r['scratch_ops']} "
              f"instructions, {r['occupancy']} waves/SIMD (radiance_kernel: {rad[F]['vgprs']}, {rad[F]['scratch']}, "
              f"{rad[F]['scratch_ops']}, {rad[F]['occupancy']})", end="")


def test_probe_eval_against_closed_forms(built):
    """sh[0] = a * 0.282095, sh[1] = b * 0.488603 / 3, the rest 0 — the probe of a radiance a + b * y — gives a + b * n_y along n (mode
    0) and a + (2/3) * b * n_y as irradiance / pi (mode 1), for normals of any length"""
    a, b = np.array([0.75, 0.85, 1.0]), np.array([-0.25, -0.15, 0.4])
    sh = np.zeros((9, 3), np.float32)
    sh[0] = a * 0.282095
    sh[1] = b * 0.488603 / 3.0
    for n in ([0, 1, 0], [0, -1, 0], [1, 0, 0], [0.3, 0.5, -0.2], [3.0, -4.0, 12.0], [-0.01, 0.002, 0.005]):
        ny = n[1] / np.linalg.norm(n)
        np.testing.assert_allclose(probe_eval(sh, n, 0), a + b * ny, rtol=1e-5, atol=0)
        np.testing.assert_allclose(probe_eval(sh, n, 1), a + (2.0 / 3.0) * b * ny, rtol=1e-5, atol=0)
    # a band-2 coefficient alone: w_2 = pi in mode 1 against 4 pi in mode 0
    sh2 = np.zeros((9, 3), np.float32)
    sh2[6] = 1.0
    np.testing.assert_allclose(probe_eval(sh2, [0, 0, 2], 0), 4 * np.pi * 0.315392 * 2.0, rtol=1e-5)
    np.testing.assert_allclose(probe_eval(sh2, [0, 0, 2], 1), np.pi * 0.315392 * 2.0, rtol=1e-5)
    # refusals: null pointers and an unknown mode, rgb untouched
    lib = ffi.load_device_lib()
    n3, rgb = (C.c_float * 3)(0, 1, 0), (C.c_float * 3)(7, 7, 7)
    p = sh.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.vk_probe_eval(None, n3, 0, rgb) == ffi.VK_ERR_BAD_ARG and lib.vk_probe_eval(p, None, 0, rgb) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_probe_eval(p, n3, 0, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_probe_eval(p, n3, 2, rgb) == ffi.VK_ERR_BAD_ARG and b"mode" in lib.vk_last_error()
    assert list(rgb) == [7, 7, 7]


def test_make_probes():
    pr = make_probes([[1, 2, 3], [4, 5, 6]], time=[0.25, 0.5])
    assert pr.dtype == RAY_DTYPE and np.isposinf(pr["tmax"]).all() and not pr["direction"].any()
    np.testing.assert_array_equal(pr["origin"], np.float32([[1, 2, 3], [4, 5, 6]]))
    np.testing.assert_array_equal(pr["time"], np.float32([0.25, 0.5]))
    assert make_probes([[0, 0, 0]], tmax=3.0)["tmax"][0] == 3.0
