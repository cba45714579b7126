"""Shade queries (vk_shade_hits, additive symbols of ABI 7) on the CPU: declared, exported by both libraries, bound, declared in the Rust
shim; the structs' sizes and offsets as gcc lays them out against the ctypes mirror and the numpy dtypes; every argument the header says
is refused, refused without a device and with the outputs untouched; no stream-taking function; the new kernel's two instances."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from vecchio_amd import build, ffi
from vecchio_amd.scene import HIT_DTYPE, PATH_STATE_DTYPE, RAY_DTYPE, SHADED_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"vk_path_state": (ffi.PathState, PATH_STATE_DTYPE), "vk_shaded": (ffi.Shaded, SHADED_DTYPE), "vk_shade_params": (ffi.ShadeParams, None)}


def header(name="vecchio_amd.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def code(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_declared_exported_and_bound(built):
    hdr = header()
    assert re.search(r"#define VK_ABI_VERSION 7\b", hdr)
    assert re.search(r"\bint vk_shade_hits\s*\(", code(hdr))
    assert "There is no device-pointer variant yet." in hdr[hdr.index("shade queries"):hdr.index("typedef struct vk_path_state")]
    for path in (ffi.device_lib_path(), build.build_device_debug()):
        lib = C.CDLL(path)
        assert hasattr(lib, "vk_shade_hits"), path
        assert not hasattr(lib, "vk_shade_hits_device"), path
    assert "vk_shade_hits" in ffi.DEVICE_SYMBOLS
    lib = ffi.load_device_lib()
    assert lib.vk_abi_version() == 7
    assert lib.vk_shade_hits.argtypes == [C.c_void_p, C.POINTER(ffi.ShadeParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                          C.POINTER(ffi.Stats)]
    assert lib.vk_shade_hits.restype is C.c_int
    assert (ffi.VK_SHADE_MISS, ffi.VK_SHADE_SCATTERED, ffi.VK_SHADE_ENDED, ffi.VK_SHADE_BAD_HIT) == (0, 1, 2, 3)
    assert re.search(r"VK_SHADE_MISS = 0, VK_SHADE_SCATTERED = 1, VK_SHADE_ENDED = 2, VK_SHADE_BAD_HIT = 3", hdr)


def test_rust_shim_declares_the_same():
    rs = open(os.path.join(ROOT, "vecchio_amd", "rust_shim", "ffi.rs")).read()
    assert re.search(r"pub fn vk_shade_hits\(scene: \*mut vk_scene, params: \*const vk_shade_params, rays: \*const vk_ray, hits: \*const vk_hit,\s*"
                     r"states: \*const vk_path_state, n: u64, out: \*mut vk_shaded, stats_out: \*mut vk_stats\) -> c_int;", rs)
    want = {
        "vk_path_state": "pub thr: [f32; 3], pub depth: u32, pub acc: [f32; 3], pub counter: u32, pub seed: u64, pub pixel: u32, pub sample: u32",
        # (nested records: the one struct of the header whose fields are structs themselves)
        "vk_shaded": "pub next: vk_ray, pub state: vk_path_state, pub status: u32, pub lobe: u32, pub _pad: [u32; 2]",
        "vk_shade_params": "pub max_depth: u32, pub integrator: u32, pub background: u32, pub background_color: [f32; 3], pub flags: u32, "
                           "pub _pad: u32",
    }
    for name, fields in want.items():
        m = re.search(r"#\[repr\(C\)\][^{;]*?pub struct " + name + r"\s*\{(.*?)\}", rs, flags=re.S)
        assert m, name
        assert " ".join(m.group(1).split()) == fields, name
    for k, v in (("VK_SHADE_MISS", 0), ("VK_SHADE_SCATTERED", 1), ("VK_SHADE_ENDED", 2), ("VK_SHADE_BAD_HIT", 3)):
        assert re.search(rf"pub const {k}: u32 = {v};", rs), k


def _walk(T, prefix=""):
    """(dotted C field path, offset within the outermost struct, size) of every leaf field of a ctypes structure"""
    for f, ft in T._fields_:
        d = getattr(T, f)
        if isinstance(ft, type) and issubclass(ft, C.Structure):
            for path, off, size in _walk(ft, prefix + f + "."):
                yield path, d.offset + off, size
        else:
            yield prefix + f, d.offset, d.size


def _dtype_offset(dt, path):
    off = 0
    for part in path.split("."):
        sub, o = dt.fields[part][:2]
        off, dt = off + o, sub
    return off, dt.itemsize


def test_struct_layout_as_gcc_sees_it(tmp_path):
    """sizes 48 / 96 / 32 and every field's offset and size, nested ones included: the header through gcc against the ctypes mirror and
    the numpy dtypes"""
    lines = []
    for cname, (T, _) in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for path, _, _ in _walk(T):
            lines.append(f'printf("{cname}.{path} %zu %zu\\n", offsetof({cname}, {path}), sizeof((({cname} *)0)->{path}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vecchio_amd.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    seen = {}
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if ln:
            k, *v = ln.split()
            seen[k] = tuple(int(x) for x in v)
    assert seen["vk_path_state"] == (48,) and seen["vk_shaded"] == (96,) and seen["vk_shade_params"] == (32,)
    n = 0
    for cname, (T, dt) in STRUCTS.items():
        assert C.sizeof(T) == seen[cname][0]
        if dt is not None:
            assert dt.itemsize == seen[cname][0]
        for path, off, size in _walk(T):
            assert seen[f"{cname}.{path}"] == (off, size), (cname, path)
            if dt is not None:
                assert _dtype_offset(dt, path) == (off, size), (cname, path)
            n += 1
    assert n == 7 + (4 + 7 + 3) + 6
    # the words the kernel reads and writes: next at 0, state at 32, status at 80
    assert seen["vk_shaded.next.origin"][0] == 0 and seen["vk_shaded.state.thr"][0] == 32 and seen["vk_shaded.status"][0] == 80


def params(**over):
    kw = dict(max_depth=5, integrator=ffi.VK_INTEGRATOR_SCATTER, background=ffi.VK_BACKGROUND_SKY, background_color=ffi.F3(0, 0, 0), flags=0,
              _pad=0)
    kw.update(over)
    return ffi.ShadeParams(**kw)


def test_bad_arguments_refused_without_a_device(built):
    lib = ffi.load_device_lib()
    sp = params()
    rays, hits, states = np.zeros(4, RAY_DTYPE), np.zeros(4, HIT_DTYPE), np.zeros(4, PATH_STATE_DTYPE)
    out = np.zeros(4, SHADED_DTYPE)
    out.view(np.uint8)[:] = 0x77
    st = ffi.Stats()
    st.samples = 99
    scene = C.c_void_p(0x1000)            # never read: each of these is refused first
    r, h, s, o = rays.ctypes.data, hits.ctypes.data, states.ctypes.data, out.ctypes.data
    cases = [
        ((None, C.byref(sp), r, h, s, 4, o), b"null argument (scene or shade parameters)"),
        ((scene, None, r, h, s, 4, o), b"null argument (scene or shade parameters)"),
        ((scene, C.byref(sp), None, h, s, 4, o), b"null rays or shaded"),
        ((scene, C.byref(sp), r, None, s, 4, o), b"null rays or shaded"),
        ((scene, C.byref(sp), r, h, None, 4, o), b"null rays or shaded"),
        ((scene, C.byref(sp), r, h, s, 4, None), b"null rays or shaded"),
        ((scene, C.byref(sp), r, h, s, 2 ** 32 + 1, o), b"2^32"),
        ((scene, C.byref(params(flags=1)), r, h, s, 4, o), b"shade flags must be 0"),
        ((scene, C.byref(params(integrator=2)), r, h, s, 4, o), b"bad integrator/background"),
        ((scene, C.byref(params(background=2)), r, h, s, 4, o), b"bad integrator/background"),
    ]
    for args, word in cases:
        assert lib.vk_shade_hits(*args, C.byref(st)) == ffi.VK_ERR_BAD_ARG, word
        assert word in lib.vk_last_error(), lib.vk_last_error()
    # outputs untouched
    assert st.samples == 99 and (out.view(np.uint8) == 0x77).all()
    # n = 2^32 itself is not refused for its size (refused here for another reason only: flags)
    assert lib.vk_shade_hits(scene, C.byref(params(flags=2)), r, h, s, 2 ** 32, o, C.byref(st)) == ffi.VK_ERR_BAD_ARG
    assert b"flags" in lib.vk_last_error()
    # no items: VK_OK, nothing done, also with null arrays (the scene handle is not read); stats zeroed
    assert lib.vk_shade_hits(scene, C.byref(sp), None, None, None, 0, None, C.byref(st)) == ffi.VK_OK and st.samples == 0
    assert lib.vk_shade_hits(scene, C.byref(sp), None, None, None, 0, None, None) == ffi.VK_OK
    assert (out.view(np.uint8) == 0x77).all()


def test_no_shade_function_takes_a_stream():
    for name in ("vecchio_amd.h", "vecchio_amd_debug.h"):
        src = code(header(name))
        decls = re.findall(r"\b(?:int|void|size_t|const char \*)\s*(vk_\w*shade\w*)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        if name == "vecchio_amd.h":
            assert [d[0] for d in decls] == ["vk_shade_hits"]
        for fn, args in decls:
            assert "stream" not in args and "void *" not in args.replace("const void *", ""), fn


def test_the_kernel_is_new_and_has_its_two_instances(built):
    """shade_hits_kernel<F>: every scene feature, with and without the PDF integrator — exactly two blocks, no AGPRs, no dynamic stack, no
    static LDS"""
    txt = open(build.kernel_resources_path()).read()
    seen = {}
    for blk in txt.split("Name: ")[1:]:
        if "shade_hits_kernel" not in blk.split("\n")[0]:
            continue
        m = re.search(r"shade_hits_kernelILj(\d+)EE", blk.split("\n")[0])
        assert m, blk.split("\n")[0]
        get = lambda k: int(re.search(re.escape(k) + r": (-?\d+)", blk).group(1))
        assert int(m.group(1)) not in seen
        seen[int(m.group(1))] = dict(vgprs=get("VGPRs"), agprs=get("AGPRs"), occupancy=get("Occupancy [waves/SIMD]"),
                                     static_lds=get("LDS Size [bytes/block]"), dynamic_stack="Dynamic Stack: True" in blk)
    assert set(seen) == {0x17F, 0x17F | 0x80}, sorted(seen)
    for F, r in seen.items():
        assert r["agprs"] == 0 and r["static_lds"] == 0 and not r["dynamic_stack"] and r["occupancy"] >= 1, (F, r)
    # the names existing tests count stay out of the new kernel's
    assert not re.search(r"irradiance|radiance_kernelILj", "".join(b.split("\n")[0] for b in txt.split("Name: ")[1:] if "shade_hits" in b))
