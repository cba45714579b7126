"""The denoiser (vk_denoise, vk_progress_stderr_device: additive symbols of ABI 7) on the CPU: declared, exported by both libraries, bound,
declared in the Rust shim, refused without a device when the arguments are bad, the documented defaults, the kernels' register budget —
and self-tests of the numpy reference (tests/denoise_ref.py) against closed forms, so that it is a reference and not a copy of the kernel."""
import ctypes as C
import os
import re

import numpy as np

import denoise_ref as R
from vecchio_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("vk_denoise_default_params", "vk_denoise", "vk_denoise_device", "vk_progress_stderr_device")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "vecchio_amd.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 7\b", hdr)
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    for name in SYMS:
        assert re.search(rf"\bint {name}\s*\(", body), name
        assert hasattr(C.CDLL(ffi.device_lib_path()), name), name
        assert hasattr(C.CDLL(build.build_device_debug()), name), name
        assert name in ffi.DEVICE_SYMBOLS
        assert re.search(rf"pub fn {name}\(", rs), name
    for name in ("vk_debug_denoise_form", "vk_debug_denoise_last_ms"):        # the hook that selects the plain form
        assert hasattr(C.CDLL(build.build_device_debug()), name), name
    assert ffi.VK_ABI_VERSION == 7
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == 7
    DP = C.POINTER(ffi.DenoiseParams)
    assert lib.vk_denoise_default_params.argtypes == [C.c_uint32, C.c_uint32, DP]
    assert lib.vk_denoise.argtypes == [C.c_void_p, DP] + [C.c_void_p] * 6 + [C.POINTER(ffi.Stats)]
    assert lib.vk_denoise_device.argtypes == [C.c_void_p, DP] + [C.c_void_p] * 7
    assert lib.vk_progress_stderr_device.argtypes == [C.c_void_p] * 3
    for name in SYMS:
        assert getattr(lib, name).restype is C.c_int
    assert [f[0] for f in ffi.DenoiseParams._fields_] == ["width", "height", "levels", "normal_squarings", "sigma_l", "sigma_z",
                                                          "albedo_floor", "flags"]
    assert C.sizeof(ffi.DenoiseParams) == 32


def test_default_params(built):
    lib = ffi.load_device_lib()
    dp = ffi.DenoiseParams()
    assert lib.vk_denoise_default_params(640, 360, C.byref(dp)) == ffi.VK_OK
    assert (dp.width, dp.height, dp.levels, dp.normal_squarings, dp.flags) == (640, 360, 5, 7, 0)
    assert (dp.sigma_l, dp.sigma_z, dp.albedo_floor) == (4.0, 1.0, float(f32(1e-3)))
    assert lib.vk_denoise_default_params(1, 1, None) == ffi.VK_ERR_BAD_ARG
    assert R.DEFAULTS == dict(levels=5, normal_squarings=7, sigma_l=4.0, sigma_z=1.0, albedo_floor=1e-3)


def test_null_arguments_refused_without_a_device(built):
    lib = ffi.load_device_lib()
    dp = ffi.DenoiseParams()
    lib.vk_denoise_default_params(4, 4, C.byref(dp))
    buf, out = (C.c_float * 48)(), (C.c_float * 48)()
    assert lib.vk_denoise(None, C.byref(dp), buf, None, None, None, None, out, None) == ffi.VK_ERR_BAD_ARG
    assert b"null" in lib.vk_last_error()
    assert lib.vk_denoise(None, None, None, None, None, None, None, None, None) == ffi.VK_ERR_BAD_ARG
    assert lib.vk_denoise_device(None, C.byref(dp), buf, None, None, None, None, out, None) == ffi.VK_ERR_BAD_ARG
    assert b"null" in lib.vk_last_error()
    assert lib.vk_progress_stderr_device(None, buf, None) == ffi.VK_ERR_BAD_ARG
    assert b"null" in lib.vk_last_error()
    assert all(v == 0.0 for v in out)


def _resources():
    txt = open(build.kernel_resources_path()).read()
    out = {}
    for blk in txt.split("Name: ")[1:]:
        m = re.search(r"\d+(denoise_\w+_kernel|progress_stderr_kernel)E", blk.split("\n")[0])
        if not m:
            continue
        get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
        assert m.group(1) not in out, m.group(1)          # one instance each
        out[m.group(1)] = dict(vgprs=get("VGPRs"), agprs=get("AGPRs"), scratch=get("ScratchSize [bytes/lane]"),
                               occupancy=get("Occupancy [waves/SIMD]"), dynamic_stack="Dynamic Stack: True" in blk,
                               lds=get("LDS Size [bytes/block]"), scratch_ops=get("ScratchOps"))
    return out


def test_denoise_kernel_budget(built):
    v = _resources()
    assert set(v) == {"denoise_prepare_kernel", "denoise_level_plain_kernel", "denoise_level_staged_kernel", "progress_stderr_kernel"}, sorted(v)
    for name, r in v.items():
        # no spills, no dynamic stack, no AGPRs anywhere; the staged form's LDS is dynamic (dn_staged_lds_bytes), none is static
        assert r["scratch"] == 0 and r["scratch_ops"] == 0 and not r["dynamic_stack"] and r["agprs"] == 0 and r["lds"] == 0, (name, r)
        assert r["occupancy"] >= 8, (name, r)
    # measured when written: prepare 20, plain 56, staged 50, stderr 45 VGPRs (8 waves per SIMD up to 64)
    assert v["denoise_prepare_kernel"]["vgprs"] <= 24
    assert v["denoise_level_plain_kernel"]["vgprs"] <= 64
    assert v["denoise_level_staged_kernel"]["vgprs"] <= 64
    assert v["progress_stderr_kernel"]["vgprs"] <= 48


# render_kernel<F, LDS_SCENE, MINW, STATS, COST, GRID> as the product library held them before the denoiser (mangled template arguments)
RENDER_INSTANCES = """
Lj0ELb0ELi7ELb0ELb0ELb0E Lj0ELb0ELi7ELb0ELb0ELb1E Lj0ELb0ELi7ELb0ELb1ELb0E Lj0ELb0ELi7ELb0ELb1ELb1E Lj0ELb1ELi6ELb0ELb0ELb0E
Lj0ELb1ELi6ELb0ELb0ELb1E Lj0ELb1ELi6ELb0ELb1ELb0E Lj0ELb1ELi6ELb0ELb1ELb1E Lj0ELb1ELi7ELb0ELb0ELb0E Lj0ELb1ELi7ELb0ELb0ELb1E
Lj128ELb0ELi7ELb0ELb0ELb0E Lj128ELb0ELi7ELb0ELb1ELb0E Lj128ELb1ELi6ELb0ELb0ELb0E Lj128ELb1ELi6ELb0ELb1ELb0E Lj128ELb1ELi7ELb0ELb0ELb0E
Lj278ELb0ELi6ELb0ELb0ELb0E Lj278ELb0ELi6ELb0ELb1ELb0E Lj278ELb1ELi6ELb0ELb0ELb0E Lj278ELb1ELi6ELb0ELb1ELb0E
Lj383ELb0ELi6ELb0ELb0ELb0E Lj383ELb0ELi6ELb0ELb1ELb0E Lj383ELb1ELi6ELb0ELb0ELb0E Lj383ELb1ELi6ELb0ELb1ELb0E
Lj406ELb0ELi6ELb0ELb0ELb0E Lj406ELb0ELi6ELb0ELb1ELb0E Lj406ELb1ELi6ELb0ELb0ELb0E Lj406ELb1ELi6ELb0ELb1ELb0E
Lj511ELb0ELi6ELb0ELb0ELb0E Lj511ELb0ELi6ELb0ELb1ELb0E Lj511ELb1ELi6ELb0ELb0ELb0E Lj511ELb1ELi6ELb0ELb1ELb0E
"""


def test_no_render_or_aov_kernel_instance_added(built):
    """the library gained kernels; the megakernel's and the AOV kernel's instances are the ones it had"""
    txt = open(build.kernel_resources_path()).read()
    names = [blk.split("\n")[0].strip() for blk in txt.split("Name: ")[1:]]
    render = sorted(m.group(1) for n in names for m in [re.search(r"render_kernelI(\w+?)EEvNS", n)] if m)
    aov = sorted(m.group(1) for n in names for m in [re.search(r"aov_kernelILj(\d+)E", n)] if m)
    assert aov == ["0", "383"], aov
    assert render == sorted(RENDER_INSTANCES.split()), render
    assert not any("DnArgs" in n and ("render_kernel" in n or "aov_kernel" in n) for n in names)


# ---------------------------------------------------------------- self-tests of the numpy reference against closed forms
def _guides(h, w, seed=1):
    g = R.synthetic(w, h, seed=seed, invalid=False)
    return dict(stderr3=g["stderr3"], normal=g["normal"], depth=g["depth"])


def test_ref_constant_power_of_two_image_is_a_fixed_point():
    h, w = 19, 23
    for value in (0.5, 4.0):
        color = np.full((h, w, 3), value, f32)
        for levels in (1, 3, 6):
            out = R.denoise(color, **_guides(h, w), levels=levels)
            np.testing.assert_array_equal(bits(out), bits(color))       # every w * I is an exact scaling, and sum(w I) / sum(w) = I


def test_ref_texture_survives_demodulation():
    h, w = 24, 24
    ys, xs = np.mgrid[0:h, 0:w]
    albedo = np.where(((xs // 3 + ys // 3) % 2 == 0)[..., None], f32([0.9, 0.5, 0.25]), f32([0.1, 0.3, 0.7])).astype(f32)
    color = (albedo * f32(0.5)).astype(f32)
    flat = dict(stderr3=np.full((h, w, 3), 0.01, f32), normal=np.broadcast_to(f32([0, 0, 1]), (h, w, 3)).copy(), depth=np.full((h, w), 3.0, f32))
    out = R.denoise(color, albedo=albedo, **flat)
    ulp = np.abs(bits(out).astype(np.int64) - bits(color).astype(np.int64))
    assert ulp.max() <= 1, ulp.max()
    # without demodulation the same filter blurs the checker
    assert np.abs(R.denoise(color, **flat, sigma_l=1e30) - color).max() > 0.05


def _halves_are_isolated(make_guides):
    h, w = 20, 32
    rng = np.random.default_rng(5)
    left = np.broadcast_to(np.arange(w)[None, :] < w // 2, (h, w))
    a = rng.random((h, w, 3)).astype(f32)
    b = a.copy()
    b[~left] = rng.random((h, w, 3)).astype(f32)[~left] * f32(7)        # other colours on the right half
    guides = make_guides(h, w, left)
    kw = dict(levels=5, sigma_l=1e30)                                    # the colour term (almost) off: only the guide isolates
    oa, ob = R.denoise(a, stderr3=np.full((h, w, 3), 0.1, f32), **guides, **kw), R.denoise(b, stderr3=np.full((h, w, 3), 0.1, f32), **guides, **kw)
    np.testing.assert_array_equal(bits(oa[left]), bits(ob[left]))
    assert (oa[~left] != ob[~left]).any()
    assert np.abs(oa[left] - a[left]).max() > 1e-3                       # and the left half was filtered


def test_ref_isolation_by_orthogonal_normals():
    _halves_are_isolated(lambda h, w, left: dict(normal=np.where(left[..., None], f32([0, 0, 1]), f32([1, 0, 0])).astype(f32)))


def test_ref_isolation_by_infinite_depth():
    _halves_are_isolated(lambda h, w, left: dict(depth=np.where(left, f32(4.0), f32(np.inf)).astype(f32)))


def test_ref_isolation_by_missing_normal():
    _halves_are_isolated(lambda h, w, left: dict(normal=np.where(left[..., None], f32([0, 0, 1]), f32([0, 0, 0])).astype(f32)))


def test_ref_invalid_pixel_is_inert():
    h, w = 17, 21
    g = R.synthetic(w, h, seed=3, invalid=False)
    a = {k: v.copy() for k, v in g.items()}
    b = {k: v.copy() for k, v in g.items()}
    a["color"][8, 10] = f32([np.nan, 1.0, 2.0])
    b["color"][8, 10] = f32([5.0, np.inf, -3.0])
    oa, ob = R.denoise(**a), R.denoise(**b)
    np.testing.assert_array_equal(bits(oa[8, 10]), bits(a["color"][8, 10]))
    np.testing.assert_array_equal(bits(ob[8, 10]), bits(b["color"][8, 10]))
    mask = np.ones((h, w), bool)
    mask[8, 10] = False
    np.testing.assert_array_equal(bits(oa[mask]), bits(ob[mask]))
    # and it is not merely a weight of zero: the neighbours differ from the frame in which the pixel is valid
    assert (R.denoise(**g)[mask] != oa[mask]).any()


def test_ref_variance_propagation_on_flat_noise():
    h = w = 200
    sigma = 0.25
    rng = np.random.default_rng(11)
    color = (f32(2.0) + f32(sigma) * rng.standard_normal((h, w, 3))).astype(f32)
    color[..., 1] = color[..., 0]
    color[..., 2] = color[..., 0]                    # grey: the luminance IS the pixel (weights sum to 1)
    flat = dict(stderr3=np.full((h, w, 3), sigma, f32), normal=np.broadcast_to(f32([0, 0, 1]), (h, w, 3)).copy(), depth=np.full((h, w), 3.0, f32))
    out, steps = R.denoise(color, **flat, levels=1, sigma_l=1e30, trace=True)
    V1 = steps[0][1]
    want = 0.2734375 ** 2 * sigma ** 2               # (sum k^2)^2 sigma^2: sum k^2 = 9/64 + 2/16 + 2/256
    np.testing.assert_allclose(V1[2:-2, 2:-2], want, rtol=1e-5)
    sample = out[4:-4:5, 4:-4:5, 0].astype(np.float64).ravel()       # footprints 5 apart: disjoint, hence independent
    N = sample.size
    est = sample.var(ddof=1)
    assert abs(est / want - 1.0) < 5.0 * np.sqrt(2.0 / N), (est, want, N)


def test_ref_falloff():
    assert R.falloff(f32(0)) == 1 and R.falloff(f32(8)) == 0 and R.falloff(f32(1e9)) == 0
    assert R.falloff(f32(np.nan)) == 0                                 # fmaxf drops the NaN
    x = np.linspace(0, 10, 4001).astype(f32)
    e = R.falloff(x)
    assert (np.diff(e) <= 0).all() and e.dtype == f32
    np.testing.assert_allclose(e[x < 1], np.exp(-x[x < 1].astype(np.float64)), atol=0.03)      # what it stands in for
