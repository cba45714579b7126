"""Temporal accumulation (vk_temporal_*: additive symbols of ABI 7) on the CPU: declared, exported by both libraries, bound, declared in
the Rust shim, struct sizes against a C compile, the documented defaults, bad arguments refused without a device, the kernel's register
budget — and self-tests of the numpy reference (tests/temporal_ref.py) against closed forms, so that it is a reference and not a copy of
the kernel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import temporal_ref as R
from vecchio_amd import HostScene, build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("vk_temporal_default_params", "vk_temporal_create", "vk_temporal_accumulate", "vk_temporal_accumulate_device", "vk_temporal_reset",
        "vk_temporal_get_info")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vecchio_amd.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 7\b", hdr)
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    for name in SYMS + ("vk_temporal_destroy",):
        assert re.search(rf"\b(int|void)\s+{name}\s*\(", body), name
        assert hasattr(C.CDLL(ffi.device_lib_path()), name), name
        assert hasattr(C.CDLL(build.build_device_debug()), name), name
        assert name in ffi.DEVICE_SYMBOLS
        assert re.search(rf"pub fn {name}\(", rs), name
    assert "pub struct vk_temporal_params" in rs and "pub struct vk_temporal_info" in rs
    lib = ffi.load_device_lib()
    assert ffi.VK_ABI_VERSION == 7 and lib.vk_abi_version() == 7
    TP = C.POINTER(ffi.TemporalParams)
    assert lib.vk_temporal_default_params.argtypes == [C.c_uint32, C.c_uint32, TP]
    assert lib.vk_temporal_create.argtypes == [C.c_void_p, TP, C.POINTER(C.c_void_p)]
    assert lib.vk_temporal_accumulate.argtypes == [C.c_void_p, C.POINTER(ffi.Camera)] + [C.c_void_p] * 8 + [C.POINTER(ffi.Stats)]
    assert lib.vk_temporal_accumulate_device.argtypes == [C.c_void_p, C.POINTER(ffi.Camera)] + [C.c_void_p] * 9
    assert lib.vk_temporal_get_info.argtypes == [C.c_void_p, C.POINTER(ffi.TemporalInfo)]
    for name in SYMS:
        assert getattr(lib, name).restype is C.c_int
    assert lib.vk_temporal_destroy.restype is None
    assert [f[0] for f in ffi.TemporalParams._fields_] == ["width", "height", "max_history", "depth_tol", "normal_cos_min", "albedo_floor",
                                                           "flags"]
    assert [f[0] for f in ffi.TemporalInfo._fields_] == ["frames", "width", "height", "pixels_with_history"]


def test_struct_sizes_against_a_c_compile(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vecchio_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(vk_temporal_params), sizeof(vk_temporal_info),\n'
                   '    offsetof(vk_temporal_params, albedo_floor), offsetof(vk_temporal_info, pixels_with_history)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(ffi.TemporalParams), C.sizeof(ffi.TemporalInfo), ffi.TemporalParams.albedo_floor.offset,
                   ffi.TemporalInfo.pixels_with_history.offset]
    assert got[:2] == [28, 24]


def test_default_params(built):
    lib = ffi.load_device_lib()
    tp = ffi.TemporalParams()
    assert lib.vk_temporal_default_params(640, 360, C.byref(tp)) == ffi.VK_OK
    assert (tp.width, tp.height, tp.max_history, tp.flags) == (640, 360, 32, 0)
    assert (tp.depth_tol, tp.normal_cos_min, tp.albedo_floor) == (float(f32(0.02)), float(f32(0.9)), float(f32(1e-3)))
    assert lib.vk_temporal_default_params(2, 2, None) == ffi.VK_ERR_BAD_ARG
    assert R.DEFAULTS == dict(max_history=32, depth_tol=0.02, normal_cos_min=0.9, albedo_floor=1e-3)
    hdr = open(os.path.join(ROOT, "include", "vecchio_amd.h")).read()
    assert "max_history 32, depth_tol 0.02, normal_cos_min 0.9, albedo_floor 1e-3" in hdr


def test_bad_arguments_refused_without_a_device(built):
    lib = ffi.load_device_lib()
    tp = ffi.TemporalParams()
    lib.vk_temporal_default_params(4, 4, C.byref(tp))
    h = C.c_void_p(0x1234)
    assert lib.vk_temporal_create(None, C.byref(tp), C.byref(h)) == ffi.VK_ERR_BAD_ARG and h.value == 0x1234
    assert b"null" in lib.vk_last_error()
    assert lib.vk_temporal_create(None, None, C.byref(h)) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_temporal_create(None, C.byref(tp), None) == ffi.VK_ERR_BAD_ARG
    nan, inf = float("nan"), float("inf")
    bad = [dict(width=1), dict(height=1), dict(width=0), dict(width=65536), dict(width=65535, height=65535), dict(max_history=0),
           dict(max_history=65536), dict(flags=1), dict(normal_cos_min=1.5), dict(normal_cos_min=-1.5), dict(normal_cos_min=nan)]
    for field in ("depth_tol", "albedo_floor"):
        bad += [{field: v} for v in (0.0, -1.0, nan, inf)]
    for over in bad:
        lib.vk_temporal_default_params(4, 4, C.byref(tp))
        for k, v in over.items():
            setattr(tp, k, v)
        assert lib.vk_temporal_create(None, C.byref(tp), C.byref(h)) == ffi.VK_ERR_BAD_ARG, over
        assert b"null" not in lib.vk_last_error(), over          # refused for the parameter, before the scene is looked at
        assert h.value == 0x1234
    cam = ffi.Camera()
    buf, out = (C.c_float * 48)(), (C.c_float * 48)()
    assert lib.vk_temporal_accumulate(None, C.byref(cam), buf, None, None, buf, buf, out, None, None, None) == ffi.VK_ERR_BAD_ARG
    assert b"null" in lib.vk_last_error()
    assert lib.vk_temporal_accumulate_device(None, C.byref(cam), buf, None, None, buf, buf, out, None, None, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_temporal_reset(None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_temporal_get_info(None, None) == ffi.VK_ERR_BAD_ARG
    lib.vk_temporal_destroy(None)
    assert all(v == 0.0 for v in out)


def _resources():
    txt = open(build.kernel_resources_path()).read()
    out = {}
    for blk in txt.split("Name: ")[1:]:
        m = re.search(r"\d+(temporal_\w+_kernel)E", blk.split("\n")[0])
        if not m:
            continue
        get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
        assert m.group(1) not in out, m.group(1)          # one instance each
        out[m.group(1)] = dict(vgprs=get("VGPRs"), agprs=get("AGPRs"), scratch=get("ScratchSize [bytes/lane]"),
                               occupancy=get("Occupancy [waves/SIMD]"), dynamic_stack="Dynamic Stack: True" in blk,
                               lds=get("LDS Size [bytes/block]"), scratch_ops=get("ScratchOps"))
    return out


def test_temporal_kernel_budget(built):
    v = _resources()
    assert set(v) == {"temporal_accumulate_kernel"}, sorted(v)
    r = v["temporal_accumulate_kernel"]
    assert r["scratch"] == 0 and r["scratch_ops"] == 0 and not r["dynamic_stack"] and r["agprs"] == 0 and r["lds"] == 0, r
    assert r["occupancy"] >= 8, r
    assert r["vgprs"] <= 64, r                  # 54 when written (8 waves per SIMD up to 64)
    assert not re.search(r"denoise_\w+_kernel|progress_stderr_kernel", "temporal_accumulate_kernel")


# ---------------------------------------------------------------- self-tests of the numpy reference against closed forms
W, H = 64, 36


def _flat(value=1.0, z=5.0, normal=(0.0, 0.0, 1.0), sigma=0.125, w=W, h=H):
    return dict(color=np.full((h, w, 3), value, f32), stderr3=np.full((h, w, 3), sigma, f32), albedo=None,
                normal=np.broadcast_to(f32(normal), (h, w, 3)).copy(), depth=np.full((h, w), z, f32))


def test_ref_own_points_project_onto_their_own_pixels():
    """a frame's first-hit points projected into its own camera give the pixel's own coordinates: on the random_spheres_demo camera at
    256x144 within 1e-3 px (6e-5 px when written)"""
    hs = HostScene("random_spheres_demo", 1)
    cam = hs.next_camera()
    w, h = 256, 144
    d = R.first_hit_dirs(cam, w, h)
    rng = np.random.default_rng(3)
    z = (f32(0.5) + f32(30) * rng.random((h, w)).astype(f32)).astype(f32)
    e = (R.vec(cam.origin) + d * (z / np.sqrt(R.dot(d, d)))[..., None]) - R.vec(cam.origin)
    for pts in (e.astype(f32), d):                                  # hits, and misses (points at infinity)
        px, py, ok = R.project(pts, cam, w, h)
        ys, xs = np.mgrid[0:h, 0:w]
        assert ok.all()
        err = max(np.abs(px - xs).max(), np.abs(py - ys).max())
        print("self-projection error", err)
        assert err <= 1e-3, err


def test_ref_max_history_1_is_the_current_frame():
    seq = R.synthetic(37, 29, seed=1, frames=3)
    acc = R.Accumulator(37, 29, max_history=1)
    for cam, g in seq:
        c, s, n = acc.accumulate(cam, **g)
        valid = np.isfinite(g["color"]).all(-1) & np.isfinite(g["stderr3"]).all(-1)
        a = np.fmax(g["albedo"], f32(1e-3))
        np.testing.assert_array_equal(bits(c[valid]), bits(((g["color"] / a) * a)[valid]))       # k = 0, alpha = 1: I' = 0 * I_h + I
        assert set(np.unique(n)) <= {0.0, 1.0}
    assert acc.took.any()


def test_ref_constant_power_of_two_image_is_a_fixed_point():
    cam = R.orbit(20.0, aspect=W / H)
    for value in (0.5, 4.0):
        acc = R.Accumulator(W, H)
        g = _flat(value)
        for i in range(6):
            c, s, n = acc.accumulate(cam, **g)
            np.testing.assert_array_equal(bits(c), bits(g["color"]))
        assert acc.took.all()


def test_ref_history_length_counts_up_to_max_history():
    cam = R.orbit(20.0, aspect=W / H)
    acc = R.Accumulator(W, H, max_history=5)
    g = _flat()
    for i in range(8):
        c, s, n = acc.accumulate(cam, **g)
        np.testing.assert_allclose(n, min(i + 1, 5), rtol=1e-5)


def _halves(make, exchange_expected=False):
    """two halves that differ in a guide never exchange history under a camera that shifts the image by about a pixel"""
    w, h = 64, 36
    left = np.broadcast_to(np.arange(w)[None, :] < w // 2, (h, w))
    cams = [R.orbit(20.5, aspect=w / h), R.orbit(20.0, aspect=w / h)]       # (the left half reprojects to the right)
    outs = []
    for right_value in (1.0, 9.0):
        acc = R.Accumulator(w, h)
        for cam in cams:
            # a flat frame at constant depth 50 under a camera that moves 0.11 units: the expected depth of a reprojected point
            # differs from the stored one by far less than the 2 % of depth_tol
            g = _flat(1.0, z=50.0, w=w, h=h)
            g["color"][~left] = f32(right_value)
            make(g, left)
            c, s, n = acc.accumulate(cam, **g)
        outs.append((c, acc.took.copy()))
    (ca, ta), (cb, tb) = outs
    assert ta[left].mean() > 0.5                                      # the left half did find its history
    if exchange_expected:
        assert (ca[left] != cb[left]).any()
    else:
        np.testing.assert_array_equal(bits(ca[left]), bits(cb[left]))


def test_ref_halves_exchange_without_a_guide_difference():
    _halves(lambda g, left: None, exchange_expected=True)            # (so the three tests below test something)


def test_ref_isolation_by_orthogonal_normals():
    def make(g, left):
        g["normal"][~left] = f32([1.0, 0.0, 0.0])
    _halves(make)


def test_ref_isolation_by_depth():
    def make(g, left):
        g["depth"][~left] = f32(50.0 * 1.5)
    _halves(make)


def test_ref_isolation_of_hit_against_miss():
    def make(g, left):
        g["depth"][~left] = np.inf
        g["normal"][~left] = f32(0)
    _halves(make)


def test_ref_invalid_pixel_is_inert_and_leaves_no_history():
    cam = R.orbit(20.0, aspect=W / H)
    g = _flat(2.0)
    g["color"][10, 20] = f32([np.nan, 1.0, 2.0])
    g["stderr3"][11, 30, 1] = np.inf
    acc = R.Accumulator(W, H)
    acc.accumulate(cam, **_flat(2.0))
    c, s, n = acc.accumulate(cam, **g)
    np.testing.assert_array_equal(bits(c[10, 20]), bits(g["color"][10, 20]))
    np.testing.assert_array_equal(bits(s[11, 30]), bits(g["stderr3"][11, 30]))
    assert n[10, 20] == 0 and n[11, 30] == 0 and (np.delete(n.ravel(), [10 * W + 20, 11 * W + 30]) == 2).all()
    assert not acc.took[10, 20] and not acc.took[11, 30]
    c, s, n = acc.accumulate(cam, **_flat(2.0))
    # a fixed camera reprojects a pixel onto itself (to within rounding): the invalid pixel's own tap carries (almost) all the weight
    assert n[10, 20] == 1 and n[11, 30] == 1 and not acc.took[10, 20] and not acc.took[11, 30]
    assert (np.delete(n.ravel(), [10 * W + 20, 11 * W + 30]) > 2.9).all()
    assert np.isfinite(c).all() and np.isfinite(s).all()


def test_ref_pure_rotation_of_a_frame_of_misses_reprojects_by_the_analytic_angle():
    w, h = 256, 144
    lf = (3.0, 2.0, 1.0)
    theta = np.radians(1.0)
    a = R.camera(lf, (3.0, 2.0, 0.0), vfov_deg=40.0, aspect=w / h)
    b = R.camera(lf, (3.0 + np.tan(theta), 2.0, 0.0), vfov_deg=40.0, aspect=w / h)      # yawed by theta about the vertical axis
    sky = dict(color=np.ones((h, w, 3), f32), stderr3=None, albedo=None, normal=np.zeros((h, w, 3), f32), depth=np.full((h, w), np.inf, f32))
    acc = R.Accumulator(w, h)
    acc.accumulate(a, **sky)
    acc.accumulate(b, **sky)
    px, py, ok = acc.proj
    # in camera a, a direction at horizontal angle phi lands at x = tan(phi) / vw * (w - 1) + (w - 1) / 2 - 0.5 (s = x + 0.5 over w - 1)
    vw = (w / h) * 2.0 * np.tan(np.radians(40.0) / 2.0)
    ys, xs = np.mgrid[0:h, 0:w]
    row = h // 2                                                      # near the horizon: t ~ 0.5, the vertical coordinate stays
    phi_b = np.arctan(((xs[row] + 0.5) / (w - 1) - 0.5) * vw)
    want = (np.tan(phi_b + theta) / vw + 0.5) * (w - 1) - 0.5
    inside = ok[row]
    assert inside.sum() > 200
    np.testing.assert_allclose(px[row][inside], want[inside], atol=2e-2)
    assert np.abs(px[row][inside] - xs[row][inside]).min() > 3.0     # about 1 degree of a 40 x 16/9 degree view: several pixels
    assert acc.took[row][inside][2:-2].all()


def test_ref_variance_follows_sigma2_over_n_on_flat_noise():
    w = h = 128
    sigma = 0.25
    cam = R.orbit(20.0, aspect=1.0)
    rng = np.random.default_rng(11)
    acc = R.Accumulator(w, h, max_history=64)
    frames = 8
    for i in range(frames):
        g = _flat(2.0, sigma=sigma, w=w, h=h)
        noise = rng.standard_normal((h, w)).astype(f32)
        g["color"] = (f32(2.0) + f32(sigma) * noise)[..., None].repeat(3, -1).astype(f32)
        c, s, n = acc.accumulate(cam, **g)
        np.testing.assert_allclose(n, i + 1, rtol=1e-5)
        # the bilinear weights of a pixel's own tap are within rounding of 1: V' = sigma^2 / N
        np.testing.assert_allclose(s[1:-1, 1:-1] ** 2, sigma ** 2 / (i + 1), rtol=1e-3)
    sample = c[1:-1, 1:-1, 0].astype(np.float64).ravel()              # pixels are independent: each blends its own history
    est = sample.var(ddof=1)
    want = sigma ** 2 / frames
    assert abs(est / want - 1.0) < 5.0 * np.sqrt(2.0 / sample.size), (est, want, sample.size)
